/* frog_chain.h -- C ABI for applying and checking a FROG transform chain (the step after the
 * registration): what `frog` writes to transforms/<i>.json, evaluated on the GPU.
 *
 * Replaces, for forward evaluation,
 *   tools/PointsTransform.cxx:70-80      vtkGeneralTransform::TransformPoint on a point
 *   tools/CheckDiffeomorphism.cxx:67-85  InternalTransformDerivative on every voxel of a
 *                                        grid, count of negative Jacobian determinants
 * The chain is the PostMultiply concatenation the reference's readers build
 * (tools/transformIO.h:375-460): transforms are applied in listed order, a
 * vtkMatrixToLinearTransform first, then one vtkBSplineTransform per lattice.
 *
 * Arithmetic (f64 throughout, as VTK's double path; VTK itself is absent from the image,
 * so this follows its documented semantics -- parity unpinned):
 *   linear   : y = M [x 1]
 *   B-spline : u = (x - origin) / spacing, cubic uniform basis (the F0..F3 of
 *              registration/imageGroup.cxx:221-232), 4x4x4 taps, taps outside the lattice
 *              contribute zero (BorderModeZero), y = x + d(x)
 *   Jacobian : analytic, I + (basis derivative / spacing) products; the chain's Jacobian is
 *              the product of the links' Jacobians at the successive points.
 * Inverse of a B-spline link (FROG_T_BSPLINE_INVERSE): Newton's method with vtkWarpTransform's
 *              defaults (tolerance 1e-3, 500 iterations, step shortening when the residual grows);
 *              the inverse of a linear link is its inverted matrix (frog_chain_invert_links).
 *              A point that has not converged after the 500 iterations (a folded lattice) returns the last point at which
 *              the residual |T(x) - p| decreased, never a worse one than the first guess p - d(p).  A NaN or infinite
 *              coordinate returns NaN in that coordinate and, no tap being read on that axis, the other two unchanged.
 * Displacement field link (FROG_T_FIELD; an extension, the reference has no such transform): `dims`, `origin`, `spacing`
 *              describe a grid of nodes, `coeffs` holds one f32 displacement per node, x fastest -- what frog_chain_sample
 *              writes with FROG_V_F32.  Forward only, f64.  Exactly, per axis: c = (p - origin) / spacing clamped to
 *              [0, dims - 1]; cell f0 = min(floor(c), dims - 2), 0 where dims == 1; fraction f = c - f0, r = 1 - f (the last
 *              node is the last cell's fraction 1; outside the grid the edge value continues).  The eight nodes of the cell,
 *              widened to f64, are blended in the order of the reslice's trilinear rule,
 *              d = rz * (ry * (rx * a + fx * b) + fy * (rx * c + fx * d)) + fz * (ry * (...) + fy * (...)), and y = p + d.
 *              Jacobian: I + dd/dp of that interpolant inside the cell (each partial divided by the axis' spacing); the
 *              column of an axis is zero where c was clamped on that axis or dims == 1.  A NaN coordinate gives NaN.
 *              There is no inverse form: frog_chain_invert_links refuses a field link.  The inverse of a transform as a
 *              field is obtained by sampling the inverted chain (frog_chain_invert_links, then frog_chain_sample).
 */
#ifndef FROG_CHAIN_H
#define FROG_CHAIN_H

#include <stddef.h>
#include <stdint.h>

#include "frog_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FROG_T_LINEAR = 0, FROG_T_BSPLINE = 1, FROG_T_BSPLINE_INVERSE = 2, FROG_T_FIELD = 3 };

typedef struct frog_chain_link {
    int type;                   /* FROG_T_LINEAR | FROG_T_BSPLINE | FROG_T_BSPLINE_INVERSE | FROG_T_FIELD */
    double matrix[16];          /* linear: row-major 4x4                                  */
    uint32_t dims[3];           /* B-spline: control points per axis; field: nodes per axis */
    double origin[3], spacing[3];
    const float *coeffs;        /* B-spline, field: dims[0]*dims[1]*dims[2] x 3 floats, x fastest */
} frog_chain_link;

typedef struct frog_chain frog_chain;

/* Copies the links (and their coefficients) to `device`.  A lattice or a field needs a non-empty grid, non-NULL values and a
 * spacing > 0 on every axis (FROG_E_INVALID otherwise). */
int frog_chain_create(const frog_chain_link *links, uint32_t n_links, int device, frog_chain **out);
void frog_chain_destroy(frog_chain *c);
uint32_t frog_chain_num_links(const frog_chain *c);

/* out[i] = chain(in[i]), n points of 3 doubles (host arrays).  A point whose taps all lie outside a lattice (however far
 * out) passes that link unchanged; a NaN coordinate gives NaN. */
int frog_chain_apply(frog_chain *c, const double *in3n, double *out3n, size_t n);

/* Jacobian determinant of the chain at origin + (i,j,k)*spacing for every node of a dims grid
 * (CheckDiffeomorphism.cxx:67-85): number of nodes with a negative determinant and the
 * smallest determinant met.  Up to 2^40 nodes (FROG_E_INVALID above); the device work goes out in launches of at most
 * 2^31 nodes, so a grid past 2^32 nodes is counted whole. */
int frog_chain_check(frog_chain *c, const double origin[3], const double spacing[3], const uint32_t dims[3],
                     uint64_t *n_negative, double *min_determinant);

/* vtkGeneralTransform::Inverse() of a chain (tools/VolumeTransform.cxx:55-57, PointsTransform's -ti):
 * the links in reverse order, matrices inverted, lattices switched between forward and inverse
 * evaluation.  `out` receives n links (coefficient pointers are shared with `in`).  Returns
 * FROG_E_INVALID for a singular matrix, and for a chain that holds a FROG_T_FIELD link. */
int frog_chain_invert_links(const frog_chain_link *in, uint32_t n, frog_chain_link *out);

/* ---- volume reslicing (tools/VolumeTransform.cxx:119-136 = vtkImageReslice) ----------------------
 * A scalar volume on a regular grid; `data` is x-fastest, one component. */
enum { FROG_V_U8 = 0, FROG_V_I8, FROG_V_U16, FROG_V_I16, FROG_V_U32, FROG_V_I32, FROG_V_F32, FROG_V_F64 };
typedef struct frog_volume {
    uint32_t dims[3];
    double   spacing[3], origin[3];
    int      dtype;             /* FROG_V_*                                                     */
    void    *data;
} frog_volume;
static inline size_t frog_volume_voxel_bytes(int dtype)
{
    switch (dtype) {
    case FROG_V_U8: case FROG_V_I8: return 1;
    case FROG_V_U16: case FROG_V_I16: return 2;
    case FROG_V_U32: case FROG_V_I32: case FROG_V_F32: return 4;
    case FROG_V_F64: return 8;
    default: return 0;
    }
}

/* The chain sampled on a grid: a dense displacement field and the map of its Jacobian determinant.
 * For every node p = origin + (i,j,k)*spacing of a dims grid, x fastest:
 *   displacement[3*idx + r] = chain(p)[r] - p[r]     (may be NULL)
 *   determinant[idx]        = det(d chain / d p)     (may be NULL; not both NULL)
 * computed in f64 exactly as frog_chain_apply and frog_chain_check compute them (the same device code: the node is
 * origin + i * spacing, the displacement the f64 difference after the chain, the determinant the cofactor expansion along
 * the first row of the product of the links' Jacobians), stored as dtype: FROG_V_F32 is one cast of the f64 value, or
 * FROG_V_F64.  So on one grid the determinants' minimum and their count below zero are frog_chain_check's results.  With
 * `determinant` NULL no Jacobian is formed; with `displacement` NULL nothing else is stored.  Host arrays; up to 2^40
 * nodes.  The device holds one slab of the grid at a time (whole launches of at most 2^31 nodes, within 1 GiB and half of
 * the free device memory), so the host arrays may be larger than device memory.  A grid with no nodes returns FROG_OK and
 * writes nothing; the grid's spacing is not validated.  FROG_E_INVALID: a NULL chain, origin, spacing or dims; both
 * outputs NULL; a dtype other than FROG_V_F32 / FROG_V_F64; more than 2^40 nodes.
 * A FROG_V_F32 displacement array is the `coeffs` of a FROG_T_FIELD link on the same grid. */
int frog_chain_sample(frog_chain *c, const double origin[3], const double spacing[3], const uint32_t dims[3],
                      int dtype, void *displacement, void *determinant);

/* out(voxel) = source(chain(position of the voxel)): `chain` maps the output grid's space to the
 * source's (for a registration transform T of the source that is T^-1: frog_chain_invert_links).
 * `out` describes the output grid (VolumeTransform takes it from the reference volume); its
 * dtype must be the source's and its data buffer is filled.  interpolation: 0 nearest, otherwise
 * trilinear.  A sample more than half a voxel outside the source's voxel centres gives
 * `background` (VTK's default border); integer outputs are rounded half up and clamped to the
 * type's range, as vtkImageReslice does.  Exactly, in f64 with every voxel read as f64:
 * c = (chain(out.origin + i * out.spacing) - source.origin) / source.spacing; inside iff
 * -0.5 <= c <= dims - 0.5 on every axis; nearest reads voxel floor(c + 0.5); trilinear taps are
 * clamped to the volume; integers get floor(v + 0.5) clamped (-2.5 -> -2, 2.5 -> 3), floats a
 * cast.  The output may hold more than 2^32 voxels: it is filled in launches of at most 2^31. */
int frog_chain_reslice(frog_chain *c, const frog_volume *source, frog_volume *out, int interpolation, double background);

/* ---- mean and stdev of a registered group (tools/AverageVolumes.cxx; transform.sh's last two steps) ----------------
 * An accumulator of n_images volumes on `grid` (dims, origin, spacing; its dtype and data are ignored).  Per voxel and in
 * the order the volumes are added, as AverageVolumes.cxx:47-59 / :68-74 does it in f32:
 *     v = (float)value;  avg += v / n;  sq += (v * v) / n;          n = (float)n_images
 *     stdev = sqrt(sq - avg * avg)                                  correctly rounded f32 sqrt of the f32 difference
 * Where that difference rounds negative the stdev is NaN, as in the reference.  One device thread owns each voxel, no
 * atomics: the results are deterministic.  Two deviations from the reference: `sq` starts at zero (upstream never clears
 * its stdev image), and a volume whose dims differ from the grid's is an error (upstream reads past its buffer).
 * A grid above 2^31 voxels is refused (FROG_E_INVALID) before the device is touched. */
typedef struct frog_average frog_average;
int  frog_average_create(const frog_volume *grid, uint32_t n_images, int device, frog_average **out);
/* chain == NULL: `source` is already on the grid (its dims must equal the grid's) -- AverageVolumes.
 * chain != NULL: `source` is resliced onto the grid exactly as frog_chain_reslice(chain, source, out, interpolation,
 * background) would (same device code), i.e. converted to the source's type (rounded half up and clamped), then added.
 * `resliced` (may be NULL; dims the grid's, dtype the source's) receives that volume.  More than n_images calls, a chain
 * on another device or bad geometry -> FROG_E_INVALID. */
int  frog_average_add(frog_average *a, frog_chain *chain, const frog_volume *source, int interpolation, double background,
                      frog_volume *resliced);
/* After exactly n_images adds (else FROG_E_INVALID): float32 mean and stdev into grid-sized host buffers, x fastest. */
int  frog_average_finish(frog_average *a, float *mean, float *stdev);
void frog_average_destroy(frog_average *a);

/* ---- mean, stdev and count over the images that cover a voxel (an extension: the reference averages the background in) --------
 * frog_average adds `background` wherever a grid voxel lies outside an image, so the mean of a group with different fields
 * of view is dimmed and its stdev inflated where only some images overlap.  This accumulator on `grid` (dims, origin,
 * spacing; its dtype and data are ignored) adds an image only where it is VALID and counts how many were.  Three values per
 * voxel: mean f32, m2 f32, count u16; one device thread owns a voxel, images in call order, no atomics: deterministic.
 * Per valid voxel, every line one correctly rounded f32 operation (Welford's update):
 *     k = count + 1;  d = x - mean;  mean = mean + d / (float)k;  m2 = m2 + d * (x - mean);  count = k
 * m2 never decreases, so the stdev is never the root of a negative difference.
 * FROG_E_INVALID, before the device is touched: a NULL argument, an empty grid or one above 2^31 voxels. */
typedef struct frog_cover frog_cover;
int  frog_cover_create(const frog_volume *grid, int device, frog_cover **out);
/* The value x = (float)r, r the voxel frog_chain_reslice(chain, source, out, interpolation, background) stores (the same
 * device code, in the source's type: integers rounded half up and clamped); `resliced` (may be NULL; dims the grid's, dtype
 * the source's) receives r for every voxel, valid or not, and is the only place `background` shows.
 * chain != NULL: the voxel is valid iff its position after the chain passes the reslice's inside test against the source
 * (-0.5 <= c <= dims - 0.5 on every axis; NaN fails) and, with a mask, the same position passes that test against the mask's
 * own geometry and the mask voxel floor(c_mask + 0.5) is non-zero.  The chain is evaluated once per voxel.  The mask (may be
 * NULL) has any of the six integer types and its own dims, origin and spacing; negative values count as non-zero.
 * chain == NULL: the source's dims, and a mask's, must equal the grid's; every voxel is inside, and valid where the mask
 * is non-zero; `resliced` receives the source.
 * FROG_E_INVALID, before any device work: a float mask, bad geometry, a chain on another device, the 65 536th add. */
int  frog_cover_add(frog_cover *a, frog_chain *chain, const frog_volume *source, const frog_volume *mask, int interpolation,
                    double background, frog_volume *resliced);
/* After at least one add (FROG_E_INVALID before), as often as wanted, and more adds may follow: grid-sized host buffers, x
 * fastest.  Where count >= min_count: the mean as held and stdev = sqrtf(m2 / (float)count) (the population stdev of the
 * valid images); elsewhere mean = fill and stdev = 0.  `count` always receives the raw count.  min_count >= 1
 * (FROG_E_INVALID for 0).  Any output may be NULL, not all three. */
int  frog_cover_finish(frog_cover *a, uint32_t min_count, float fill, float *mean, float *stdev, uint16_t *count);
void frog_cover_destroy(frog_cover *a);

/* ---- one image against the mean of the group (which images registered badly?) -------------------------------------------------
 * Sums over the grid voxels of an image's value x and a reference y taken from the accumulator, and their joint histogram:
 * what normalised cross-correlation and mutual information are formed from (frog_score_metrics_from, frog_host.h).  The call
 * reads the accumulator and leaves mean, m2 and count as they are: it may come after any add, in any order with
 * frog_cover_finish and with further adds.
 * Per grid voxel v:
 *   valid   : exactly where frog_cover_add(a, chain, source, mask, interpolation, background, NULL) would count the voxel (the
 *             same device code: with a chain the inside test against the source, then the mask at the same position; without
 *             one equal dims, every voxel inside, the mask's own voxel).
 *   x       : (float)r, r the voxel frog_chain_reslice stores there, as in frog_cover_add.
 *   y (f64) : k = count[v], m = mean[v].
 *             leave_one_out != 0: the voxel takes part iff k >= max(2, min_count), and
 *                 y = ((double)m * (double)k - (double)x) / (double)(k - 1)         three f64 operations, no contraction
 *             -- the mean of the OTHER images, up to Welford's f32 rounding, for an image that is one of the adds.
 *             leave_one_out == 0: the voxel takes part iff k >= max(1, min_count), and y = (double)m -- for an image that is
 *             not in the accumulator (a new subject against an atlas).
 *   A valid voxel that takes part and whose x or y is not finite adds one to n_nonfinite and to nothing else.  Every other
 *   such voxel adds one to n, the six terms  (double)x, y, x * x, y * y, x * y, |x - y|  (each one f64 operation on (double)x
 *   and y) to sx, sy, sxx, syy, sxy, sad, and one to a histogram bin.
 *   histogram: scale = (float)bins / (hi - lo), formed once on the host in f32;
 *              bin(t) = min(bins - 1, max(0, floorf((t - lo) * scale))) in f32, one operation per step, the clamp applied
 *              to the float before the conversion (so +-inf, which (float)y may be, lands in the last or first bin);
 *              histogram[bin(x) * bins + bin((float)y)] += 1.  Integer counts: exact, and their sum is n.
 * The order of the f64 additions, complete (no floating-point atomic is used; the result does not depend on scheduling, on
 * the device's load or on how the work is cut into launches):
 *   1. The grid's voxels, x fastest, are cut into tiles of 2048 consecutive voxels; tile T holds voxels [2048 T, 2048 T + 2048).
 *      The last tile may be partial.
 *   2. A tile belongs to 256 threads; thread t (0..255) starts six sums at +0.0 and adds the terms of the voxels
 *      2048 T + 256 j + t for j = 0, 1, ..., 7 in that order; a voxel that adds nothing (past the grid, invalid, too few
 *      images, not finite) is skipped.
 *   3. Threads 64 w .. 64 w + 63 form wave w (0..3), thread 64 w + l being lane l.  For h = 32, 16, 8, 4, 2, 1 in turn every
 *      lane l < h replaces its sum by (its sum) + (the sum of lane l + h); lane 0 then holds the wave's sum.
 *   4. The tile's sum is ((wave 0 + wave 1) + wave 2) + wave 3.
 *   5. The result is the tiles' sums added one by one in ascending T, starting from +0.0.
 * n and n_nonfinite travel the same way as integers.
 * bins == 0 with histogram == NULL: no histogram, lo and hi are ignored.  Otherwise 2 <= bins <= 64, lo and hi finite,
 * hi > lo and hi - lo finite in f32.  `histogram` is a host array of bins * bins counts, row = x bin.
 * FROG_E_INVALID, before any device work: a NULL accumulator, source or sums; the geometry and mask errors of frog_cover_add;
 * a chain on another device; a call before the first add; min_count == 0; bins, range or histogram other than stated. */
typedef struct frog_score_sums {
    uint64_t n;             /* voxels that entered the sums and the histogram                 */
    uint64_t n_nonfinite;   /* valid, counted voxels skipped because x or y was not finite    */
    double   sx, sy, sxx, syy, sxy, sad;    /* sums of x, y, x^2, y^2, x y, |x - y|, f64      */
} frog_score_sums;
int  frog_cover_score(frog_cover *a, frog_chain *chain, const frog_volume *source, const frog_volume *mask, int interpolation,
                      double background, uint32_t min_count, int leave_one_out, uint32_t bins, float lo, float hi,
                      frog_score_sums *sums, uint64_t *histogram);

/* ---- median, MAD and quantile images of a registered group (an extension: order statistics across the images) -----------------
 * The moments above stream; an order statistic does not: this accumulator keeps every added image's value per voxel, then
 * sorts per voxel.  It holds the z-planes [first_plane, first_plane + n_planes) of `grid` (dims, origin, spacing; its dtype
 * and data are ignored): the WINDOW, n_planes * dims[1] * dims[0] voxels, x fastest.  A voxel's position is computed from
 * its index in the whole grid, with the device code of frog_cover_add (the window is not a sub-grid with a shifted origin,
 * which would round differently), so windows that partition the grid give, bit for bit, what one whole-grid window gives.
 * The device holds 4 bytes per image and window voxel; n_images x window voxels may exceed 2^32.
 *
 * frog_rank_planes: the largest n_planes the device would accept for this grid and n_images: half of the free device memory
 * at the time of the call / (4 bytes x n_images x dims[0] x dims[1]), at most dims[2]; FROG_E_INVALID when not one plane fits.
 *
 * What an add keeps.  Add number i (0-based, in call order) fills plane i of the window with one u32 per voxel:
 *   x   = (float)r, r the voxel frog_chain_reslice(chain, source, out, interpolation, background) stores there, in the
 *         source's type, as in frog_cover_add;
 *   key = ~u where the sign bit of u = bits(x) is set, else u ^ 0x80000000: unsigned order of the keys is
 *         -inf < ... < -0 < +0 < ... < +inf;
 *   the entry TAKES PART iff the voxel is valid by frog_cover_add's rule (with a chain the inside test against the source,
 *   then the mask at the same position; with chain == NULL equal dims and the mask's own voxel) and x is not NaN; every other
 *   entry holds 0xFFFFFFFF, the key of a NaN, which no participating value has and which sorts last.
 * The chain is evaluated once per voxel and add.  More than n_images adds are refused.
 *
 * What finish returns, per window voxel, after any number of adds >= 1 (more adds may follow, and finish may be called again).
 * k is the number of participating entries and a[0 .. k-1] their values in ascending key order.
 *   count = k: frog_cover's count minus the valid NaNs.
 *   Where k < min_count every quantile is `fill` and mad is 0.  Otherwise, for each of the n_q probabilities q, in f64 with one
 *   rounded operation per step and no contraction:
 *       h = q * (double)(k - 1);  lo = floor(h);  f = h - lo;  hi = min(lo + 1, k - 1)
 *       value(q) = a[lo]                                                        if f == 0 or a[lo] == a[hi] (so -0 == +0)
 *                = (float)((double)a[lo] + f * ((double)a[hi] - (double)a[lo]))  otherwise
 *   so equal neighbours never give inf - inf.  Neighbours -inf and +inf do; a NaN result is stored as 0x7FC00000.
 *   quantiles: n_q window-sized planes, plane j for q[j].
 *   mad: m = value(0.5) as the f32 it is stored as.  m not finite: mad = NaN (0x7FC00000).  Else d_i = |a[i] - m| in f32 (one
 *   rounded subtraction, then the absolute value), and mad = value(0.5) of the sorted d by the same rule.  It is the raw
 *   median absolute deviation: multiply by 1.4826 for a consistent estimate of a normal stdev.
 * Order statistics are exact: the result does not depend on the sorting method, on scheduling or on how the work is cut into
 * launches or windows.  n_q is 0..16 with every q in [0, 1] (NaN refused); any output may be NULL, not all of them (n_q == 0 or
 * quantiles == NULL: mad or count).  Host buffers, window-sized, x fastest.
 * FROG_RANK_MAX_IMAGES is the capacity of the sort kernels (one voxel's keys padded to a power of two in registers up to 64
 * images, in LDS above), not of the 16-bit counts.
 * FROG_E_INVALID, before the device is touched: a NULL argument, an empty grid or one above 2^31 voxels, a window outside the
 * grid or n_planes == 0, n_images == 0 or > FROG_RANK_MAX_IMAGES; in add a float mask, bad geometry, a chain on another
 * device, the (n_images + 1)th add; in finish min_count == 0, n_q > 16, a q outside [0, 1], no add yet. */
#define FROG_RANK_MAX_IMAGES 4096
typedef struct frog_rank frog_rank;
int  frog_rank_planes(const frog_volume *grid, uint32_t n_images, int device, uint32_t *planes);
int  frog_rank_create(const frog_volume *grid, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, int device, frog_rank **out);
int  frog_rank_add(frog_rank *a, frog_chain *chain, const frog_volume *source, const frog_volume *mask, int interpolation, double background);
int  frog_rank_finish(frog_rank *a, uint32_t min_count, float fill, uint32_t n_q, const double *q,
                      float *quantiles, float *mad, uint16_t *count);
void frog_rank_destroy(frog_rank *a);

/* ---- majority-vote fusion of a registered group's label maps (an extension: the reference stops at N x VolumeTransform -i 0) --
 * An accumulator of n_images label volumes on `grid` (dims, origin, spacing; its dtype and data are ignored).  Per voxel v
 * and label value l it counts the images that carry l at v: count[l][v], 16-bit, one device thread per voxel, no atomics on
 * the counts.  Everything that leaves it is integer arithmetic on those counts (or one f32 division): exact and independent
 * of scheduling.  The distinct values are found on the device; max_labels (0: 1024) bounds their number, and the device
 * holds one plane of 2 bytes x the grid's voxels per distinct value.
 * FROG_E_INVALID, before the device is touched: a NULL argument, an empty grid or one above 2^31 voxels, n_images == 0 or
 * > 65535 (the counters' width), max_labels > 65536. */
typedef struct frog_labels frog_labels;
int  frog_labels_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, int device, frog_labels **out);
/* `source` has one of the six integer types (FROG_E_INVALID for FROG_V_F32 / FROG_V_F64, and for a background that is not
 * finite).  chain == NULL: it is already on the grid (its dims must equal the grid's).  chain != NULL: every grid voxel gets
 * the voxel frog_chain_reslice(chain, source, out, 0, background) stores there (nearest neighbour; the same device code),
 * and `resliced` (may be NULL; dims the grid's, dtype the source's) receives that volume.  The background is a label like
 * any other.  The image's vote at v goes to the label it has there: count[label][v] += 1.  More than n_images calls, a chain
 * on another device or bad geometry -> FROG_E_INVALID.  A volume that would bring the number of distinct labels above
 * max_labels is refused with FROG_E_INVALID (the message names the limit), a refused device allocation with FROG_E_NOMEM:
 * either way the volume leaves no vote and no label behind, the call does not count as one of the n_images, and another
 * volume may be added in its place. */
int  frog_labels_add(frog_labels *a, frog_chain *chain, const frog_volume *source, double background, frog_volume *resliced);
/* After exactly n_images adds (else FROG_E_INVALID): the number of distinct labels that received a vote.  The four getters
 * below are valid only after it (FROG_E_INVALID before). */
int  frog_labels_finish(frog_labels *a, uint32_t *n_labels);
/* n_labels entries each, in ascending signed order of the values: voxels[l] = sum over v of c, pairs[l] = sum over v of
 * c (c - 1) / 2, c = count[l][v]; exact in u64.  The pooled pairwise Dice overlap of label l across the group,
 *     sum_{i<j} 2 |A_i n A_j| / sum_{i<j} (|A_i| + |A_j|)  =  2 pairs[l] / ((n_images - 1) voxels[l]),
 * because sum_{i<j} |A_i n A_j| = sum_v C(c, 2) and sum_{i<j} (|A_i| + |A_j|) = (n_images - 1) sum_i |A_i|.  Callers form the
 * quotient in f64 (undefined for n_images == 1). */
int  frog_labels_table(frog_labels *a, int64_t *values, uint64_t *voxels, uint64_t *pairs);
/* Per voxel the label with the most votes, a tie going to the smallest value (signed comparison), stored as label->dtype
 * (any of the six integer types; dims the grid's); agreement[v] = (float)c_winner / (float)n_images, one correctly rounded
 * f32 division.  Either output may be NULL, not both.  A table value that does not fit label->dtype -> FROG_E_INVALID and
 * nothing is written. */
int  frog_labels_fused(frog_labels *a, frog_volume *label, float *agreement);
/* p[v] = (float)count[value][v] / (float)n_images; a value that is not in the table -> FROG_E_INVALID. */
int  frog_labels_probability(frog_labels *a, int64_t value, float *p);
void frog_labels_destroy(frog_labels *a);

/* ---- STAPLE label fusion: an EM consensus and every image's performance (an extension; Warfield, Zou, Wells, IEEE TMI
 * 23(7), 2004, multi-label form) --------------------------------------------------------------------------------------------
 * An accumulator of n_images label volumes on `grid` (dims, origin, spacing; its dtype and data are ignored).  It keeps the
 * label of image i at voxel v as a one-byte dense index D[i][v]; after finish index l stands for the l-th distinct value in
 * ascending signed order, D[i][v] in [0, L).  solve estimates theta[i][l'][l] = P(image i shows l' | the truth is l) and
 * q[v][l], the probability that the truth at v is l, as a u32 in units of 2^-30.  Every floating-point line below is one
 * separately rounded f64 operation (no contraction, no log or exp), every sum is an exact u64 sum, and there is no
 * floating-point atomic: what leaves the library is the same bits from run to run and however the work is cut into launches.
 * Constants: FLOOR = 2^-24, ONE = 2^30, K = 16.  n = n_images, V = the grid's voxels.
 *   Active voxels: all, or with restrict_to_disputed only those at which not all n images carry the same label; A is their
 *     number.  An inactive voxel has q = ONE for its unanimous label and 0 for the others, and enters no sum below.
 *   Prior:  prior[l] = (double)c[l] / (double)(n A), c[l] the u64 number of (image, active voxel) entries that carry l.
 *   Start:  theta[i][l'][l] = p0 where l' == l, else (1.0 - p0) / (double)(L - 1).
 *   E-step, per active voxel and label l:
 *     1. m = prior[l]; e = 0
 *     2. for i ascending: m = m * max(theta[i][D[i][v]][l], FLOOR)
 *     3. after every factor with i % K == K - 1, and after the last one: (m, k) = frexp(m); e += k
 *     4. emax = the largest e over the labels with m > 0
 *     5. p[l] = ldexp(m, e - emax), which is 0 where m == 0
 *     6. s = the sum of p[l] over l ascending, from +0.0
 *     7. q[v][l] = (uint32)rint((p[l] / s) * 2^30), round half to even
 *   M-step: T[l] = sum over the active v of q[v][l]; S[i][l'][l] = sum of q[v][l] over the active v with D[i][v] == l'; both
 *     u64.  theta[i][l'][l] = (double)S[i][l'][l] / (double)T[l]; the previous value stays where T[l] == 0.
 *   Loop:  it = 0.  Repeat: E-step; stop if it == max_iter; M-step; change = the largest |theta_new - theta_old|; it += 1;
 *     if change < tol, one more E-step with the final theta, and stop.  *change is +inf when no M-step ran.  With A == 0
 *     nothing runs: 0 iterations, prior 0, theta as started.
 * Device memory: n V bytes (D) + V bytes (the active mask) + 4 L V bytes (q, which is stored, not recomputed: the M-step and
 * the getters read what the last E-step wrote) + 16 n L^2 bytes (theta and S) + the staging of one source volume and, with a
 * chain, of its resliced copy.  There are no slabs: the EM couples all voxels.
 * FROG_E_INVALID, before the device is touched: a NULL argument, an empty grid or one above 2^31 voxels, n_images == 0 or
 * > 4096, max_labels > FROG_STAPLE_MAX_LABELS (0: 256); everything frog_labels_add refuses (a float volume, a background
 * that is not finite, bad geometry, a chain on another device, the (n_images + 1)th add); p0 outside (0, 1) or NaN, tol
 * negative or NaN; a solve before finish, a getter before solve.  A refused device allocation is FROG_E_NOMEM. */
#define FROG_STAPLE_MAX_LABELS 256
typedef struct frog_staple frog_staple;
int  frog_staple_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, int device, frog_staple **out);
/* frog_labels_add's rules: one of the six integer types; chain == NULL: already on the grid; chain != NULL: nearest-neighbour
 * reslicing through the same device code, `resliced` (may be NULL) receives that volume; the background is a label like any
 * other.  A volume that would bring the distinct labels above max_labels is refused with FROG_E_INVALID and leaves nothing
 * behind: the call does not count and another volume may be added in its place. */
int  frog_staple_add(frog_staple *a, frog_chain *chain, const frog_volume *source, double background, frog_volume *resliced);
/* After exactly n_images adds (else FROG_E_INVALID): renumbers D and returns L, the number of distinct labels. */
int  frog_staple_finish(frog_staple *a, uint32_t *n_labels);
int  frog_staple_values(frog_staple *a, int64_t *values);                    /* ascending, signed */
/* The loop above; may be called again with other arguments, each call starts afresh. */
int  frog_staple_solve(frog_staple *a, double p0, double tol, uint32_t max_iter, int restrict_to_disputed,
                       uint32_t *iterations, double *change, uint64_t *active_voxels);
/* Per voxel the first label in ascending order with the strictly largest q, stored as label->dtype (any of the six integer
 * types; dims the grid's); confidence[v] = (float)((double)q_winner * 2^-30).  Either output may be NULL, not both.  A value
 * that does not fit label->dtype -> FROG_E_INVALID and nothing is written. */
int  frog_staple_fused(frog_staple *a, frog_volume *label, float *confidence);
/* p[v] = (float)((double)q[v][value] * 2^-30); a value that no image carries -> FROG_E_INVALID. */
int  frog_staple_probability(frog_staple *a, int64_t value, float *p);
/* theta and sums: n L L entries each, entry (i L + l') L + l; totals and prior: L each.  sums and totals are those of the
 * last M-step that ran (zeros if none did).  Any may be NULL, not all. */
int  frog_staple_performance(frog_staple *a, double *theta, uint64_t *sums, uint64_t *totals, double *prior);
void frog_staple_destroy(frog_staple *a);

/* ---- locally weighted label fusion: a target image segmented from a registered group (an extension; Artaechevarria et al.,
 * IEEE TMI 28(8), 2009: every atlas votes for its label with a weight that grows with its local similarity to the target) ------
 * An accumulator of n_images atlases on `grid` (dims, origin, spacing; its dtype and data are ignored).  An atlas is an image
 * and an integer label map that go through one chain; its vote at voxel v goes to the label it has there, weighted by the
 * normalised cross-correlation between its resliced image and the resliced target over the patch of v:
 * score[label][v], f32, one device thread per voxel in every plane, atlases in call order.  Every floating-point line below
 * is one separately rounded operation; there is no floating-point atomic and the results are the same bits from run to run
 * and however the work is cut into launches.
 * radius 1..4: the patch is (2 radius + 1)^3 voxels; power 1..8; floor in [0, 1]: the least similarity an atlas is credited
 * with.  max_labels (0: 1024, at most 65536) bounds the distinct label values.  Device memory: one f32 plane of 4 x the grid's
 * voxels per distinct label value, two f32 staging planes of the same size (the target and the current atlas image), and
 * the staging of the current image, label map and their resliced volumes.
 * FROG_E_INVALID, before the device is touched: a NULL argument, an empty grid or one above 2^31 voxels, n_images == 0,
 * max_labels > 65536, radius == 0 or > 4, power == 0 or > 8, floor outside [0, 1] or NaN. */
typedef struct frog_wlabels frog_wlabels;
int  frog_wlabels_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels,
                         uint32_t radius, uint32_t power, float floor, int device, frog_wlabels **out);
/* The image to segment: exactly once, before the first add (a second call, or one after an add -> FROG_E_INVALID).  `source`
 * has any of the eight types.  Per grid voxel v, t[v] = (float)r, r the voxel frog_chain_reslice(chain, source, out,
 * interpolation, background) stores (the same device code, in the source's type, as in frog_cover_add), and validT[v] iff
 * the position after the chain passes the reslice's inside test against the source (-0.5 <= c <= dims - 0.5 on every axis;
 * NaN fails) and t[v] is finite.  chain == NULL: the source's dims must equal the grid's, every voxel is inside, and valid
 * where t[v] is finite.  `resliced` (may be NULL; dims the grid's, dtype the source's) receives r for every voxel, valid or
 * not (without a chain: the source), and is the only place `background` shows.  A chain on another device, bad geometry ->
 * FROG_E_INVALID. */
int  frog_wlabels_target(frog_wlabels *a, frog_chain *chain, const frog_volume *source,
                         int interpolation, double background, frog_volume *resliced);
/* One atlas.  The chain is evaluated once per voxel for both volumes.  `image` (any of the eight types) gives a[v] = (float)r
 * and validA[v] exactly as the target's t[v] and validT[v].  `labels` (one of the six integer types; its own dims, origin and
 * spacing) gives label[v], the voxel frog_chain_reslice(chain, labels, out, 0, label_background) stores (nearest neighbour)
 * at the same position after the chain; the label background is a label like any other.  chain == NULL: both volumes have
 * the grid's dims.  `resliced_image` and `resliced_labels` (each may be NULL; dims the grid's, dtype their source's) receive
 * the two resliced volumes, as frog_chain_reslice gives them.
 *   member[u] = validT[u] && validA[u]
 *   patch(v)  = the grid voxels u with |u - v| <= radius on all three axes (voxels outside the grid do not exist) that
 *               are members
 *   six f64 sums, each from +0.0, over patch(v) with z ascending, then y, then x, T = (double)t[u], A = (double)a[u]:
 *               n += 1;  st += T;  sa += A;  stt += T * T;  saa += A * A;  sta += T * A
 *   cov = n * sta - st * sa;  vt = n * stt - st * st;  va = n * saa - sa * sa                      (f64)
 *   if n >= 2 and vt > 0 and va > 0 and cov > 0:
 *               q = (float)((cov * cov) / (vt * va));  c = sqrtf(q);  c = min(c, 1.0f) if c is finite
 *   else        c = 0
 *   c = max(c, floor)
 *   w = c;  then power - 1 times  w = w * c                                                         (f32)
 *   if member[v]:  score[label[v]][v] = score[label[v]][v] + w                                       (f32)
 * A voxel that is no member gets no vote from this atlas.  With floor == 1 every weight is exactly 1: the majority vote over
 * the atlases that cover the voxel together with the target.
 * FROG_E_INVALID, before any device work: a NULL argument, a float label volume, a background that is not finite, an add
 * before the target, more than n_images adds, a chain on another device, bad geometry.  An atlas whose label map (all grid
 * voxels of it, members or not) would bring the number of distinct labels above max_labels is refused with FROG_E_INVALID
 * (the message names the limit), a refused device allocation with FROG_E_NOMEM: either way the atlas leaves no vote and no
 * label behind, the call does not count as one of the n_images, and another atlas may be added in its place. */
int  frog_wlabels_add(frog_wlabels *a, frog_chain *chain, const frog_volume *image, const frog_volume *labels,
                      int interpolation, double image_background, double label_background,
                      frog_volume *resliced_image, frog_volume *resliced_labels);
/* After exactly n_images adds (else FROG_E_INVALID): the number of distinct label values the atlases' resliced label maps
 * hold, whether or not a vote reached them.  The four getters below are valid only after it (FROG_E_INVALID before). */
int  frog_wlabels_finish(frog_wlabels *a, uint32_t *n_labels);
int  frog_wlabels_values(frog_wlabels *a, int64_t *values);            /* ascending, signed */
/* total[v] = the f32 sum of score[l][v] over the labels in ascending signed order of their values, from +0.0.  The fused
 * label is the first value in that order whose score is strictly larger than every earlier one and > 0, stored as
 * label->dtype (any of the six integer types; dims the grid's); confidence[v] = score_winner / total, one f32 division.
 * Where total == 0 (no atlas covers the voxel together with the target, or every weight there is 0) the label is fill_label
 * and the confidence 0.  Either output may be NULL, not both.  A table value or fill_label that does not fit label->dtype ->
 * FROG_E_INVALID and nothing is written. */
int  frog_wlabels_fused(frog_wlabels *a, int64_t fill_label, frog_volume *label, float *confidence);
/* p[v] = score[value][v] / total[v], one f32 division; 0 where total == 0.  A value that is not in the table ->
 * FROG_E_INVALID. */
int  frog_wlabels_probability(frog_wlabels *a, int64_t value, float *p);
void frog_wlabels_destroy(frog_wlabels *a);

/* ---- joint label fusion (an extension; Wang, Suh, Das, Pluta, Craige, Yushkevich, IEEE PAMI 35(3), 2013: the atlases' weights
 * at a voxel minimise the expected error of the combined vote given how the atlases' errors correlate over the patch, so
 * atlases that are wrong in the same way share one vote) ------------------------------------------------------------------------
 * An accumulator of n_images <= 32 atlases on `grid`, as frog_wlabels.  An add only collects: the atlas' f32 plane (NaN where
 * not valid) and its resliced label map stay on the device until frog_jlabels_finish, which solves one n x n system per voxel
 * and votes.  Every floating-point line below is one separately rounded f64 operation unless marked; there is no
 * floating-point atomic and the results are the same bits from run to run and however the work is cut into launches.
 * radius 1..3: the patch is (2 radius + 1)^3 voxels; beta 1..4, an integer, the elementwise power of the Gram matrix (which
 * stays positive semidefinite: Schur product theorem); alpha > 0, finite, added to the diagonal; max_labels as frog_wlabels.
 * Device memory, V the grid's voxels: n_images x (4 V for the image plane + V x the label type's bytes for its label map,
 * allocated by the add) + 4 V for the target + 4 V per distinct label value; with keep_weights n_images x 4 V more; and the
 * staging of the current image, label map and resliced image.  There is no cutting into slabs: a grid whose planes do not
 * fit is refused with FROG_E_NOMEM by the call that allocates.
 * FROG_E_INVALID, before the device is touched: everything frog_wlabels_create refuses for grid, n_images and max_labels,
 * n_images > 32, radius == 0 or > 3, beta == 0 or > 4, alpha not finite or <= 0. */
typedef struct frog_jlabels frog_jlabels;
int  frog_jlabels_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, uint32_t radius, uint32_t beta,
                         double alpha, int keep_weights, int device, frog_jlabels **out);
/* Exactly frog_wlabels_target: t[v] and validT[v]. */
int  frog_jlabels_target(frog_jlabels *a, frog_chain *chain, const frog_volume *source,
                         int interpolation, double background, frog_volume *resliced);
/* Exactly frog_wlabels_add's arguments, a_i[v], validA_i[v], label_i[v], resliced volumes, refusals and the take-back of a
 * refused atlas; no vote yet. */
int  frog_jlabels_add(frog_jlabels *a, frog_chain *chain, const frog_volume *image, const frog_volume *labels,
                      int interpolation, double image_background, double label_background,
                      frog_volume *resliced_image, frog_volume *resliced_labels);
/* After exactly n_images adds (else FROG_E_INVALID): solves and votes, then returns the number of distinct label values as
 * frog_wlabels_finish.  At grid voxel v, patch(v) = the grid voxels u with |u - v| <= radius on all three axes (voxels
 * outside the grid do not exist), walked with z ascending, then y, then x:
 *   Patch statistics, for X = t and for X = every a_i, over the u of patch(v) where X is valid, each sum from +0.0:
 *               x = (double)X[u];  n = n + 1;  s = s + x;  xx = x * x;  ss = ss + xx
 *               nss = n * ss;  s2 = s * s;  num = nss - s2;  nn = n * n;  var = num / nn;  mean = s / n
 *               if n >= 2 and var > 0:  sd = sqrt(var);  inv = 1 / sd        else  inv = 0
 *   Differences, where validT[u] and validA_i[u]:
 *               ac = (double)a_i[u] - mean_i;  ah = ac * inv_i;  tc = (double)t[u] - mean_t;  th = tc * inv_t
 *               e = ah - th;  d_i(u) = fabs(e)                               elsewhere  d_i(u) = +0.0
 *   Gram matrix, for j <= i, each entry from +0.0, over patch(v) in the stated order:
 *               p = d_i(u) * d_j(u);  M[i][j] = M[i][j] + p
 *   Power:      K[i][j] = M[i][j];  then beta - 1 times  K[i][j] = K[i][j] * M[i][j];  then  K[i][i] = K[i][i] + alpha
 *   Active set: atlas i is active at v iff validT[v] && validA_i[v].  The system is K restricted to the active atlases in call
 *               order; an atlas that is not active has weight 0 and no vote; no active atlas, or a target that is not valid
 *               at v: no score is written at v.
 *   K w = 1 by LDL^T without pivoting (loops ascending unless said otherwise):
 *     for j:    D_j = K_jj;  for k < j:  q = L_jk * L_jk;  m = q * D_k;  D_j = D_j - m
 *               for i > j:   x = K_ij;  for k < j:  q = L_ik * L_jk;  m = q * D_k;  x = x - m;   then  L_ij = x / D_j
 *     forward:  z_i = 1;  for k < i:  m = L_ik * z_k;  z_i = z_i - m
 *     diagonal: y_i = z_i / D_i
 *     backward, i descending:  w_i = y_i;  for k > i ascending:  m = L_ki * w_k;  w_i = w_i - m
 *     normalise: S = +0.0;  for i:  S = S + w_i;   then  w_i = w_i / S;  the weight of atlas i at v is (float)w_i
 *   Votes, in call order over the active atlases:  score[label_i[v]][v] = score[label_i[v]][v] + (float)w_i          (f32)
 * Weights may be negative: that is the method, and how it cancels an error the atlases share.  They are neither clamped nor
 * renormalised.  The four getters below are valid only after finish (FROG_E_INVALID before). */
int  frog_jlabels_finish(frog_jlabels *a, uint32_t *n_labels);
int  frog_jlabels_values(frog_jlabels *a, int64_t *values);            /* ascending, signed */
/* Exactly frog_wlabels_fused on these scores: total in ascending label order, the winner the first strictly larger score
 * that is > 0, confidence = winner / total, fill_label and 0 where total == 0.  Where other labels' scores are negative the
 * total is smaller than the winner's score and the confidence exceeds 1. */
int  frog_jlabels_fused(frog_jlabels *a, int64_t fill_label, frog_volume *label, float *confidence);
int  frog_jlabels_probability(frog_jlabels *a, int64_t value, float *p);       /* as frog_wlabels_probability */
/* w[v] = the weight of atlas image_index (in call order) at v, 0 where it is not active.  Without keep_weights, before
 * finish, or image_index >= n_images -> FROG_E_INVALID. */
int  frog_jlabels_weight(frog_jlabels *a, uint32_t image_index, float *w);
void frog_jlabels_destroy(frog_jlabels *a);

/* ---- surface distances between label maps: an exact Euclidean distance transform (an extension; the reference has no
 * counterpart) ---------------------------------------------------------------------------------------------------------------
 * How far apart are the boundaries of a structure in two label maps, in the spacing's unit: the Hausdorff distance, a
 * percentile of it and the average symmetric surface distance.  Every line below is one separately rounded f64 operation or an
 * integer operation (no contraction), every sum, maximum and order statistic is integer arithmetic: what leaves the library is
 * the same bits from run to run and however the work is cut into launches.
 *   Surface.  For a label map m on a grid and a value l, A = {v : m[v] == l}.  A voxel of A is a SURFACE VOXEL if at least one
 *     of its six face neighbours is not in A; a neighbour outside the grid counts as not in A.
 *   Distance transform of a voxel set F (the features) at spacing (sx, sy, sz):
 *     g1[x,y,z] = min over q of ( F[q,y,z] ? ((double)(x - q) * sx)^2 : +inf )
 *     g2[x,y,z] = min over q of ( g1[x,q,z] + ((double)(y - q) * sy)^2 )
 *     g3[x,y,z] = min over q of ( g2[x,y,q] + ((double)(z - q) * sz)^2 )
 *     d * d is one multiplication, the + one addition.  The minimum of f64 values does not depend on the order it is taken in,
 *     so every method that returns the true minimum of these expressions returns these bits.
 *   Stored distance: unsigned 32-bit fixed point in units of 2^-16 of the spacing's unit,
 *     u = (g3 == +inf) ? 0xFFFFFFFF : min(0xFFFFFFFE, (uint64)llrint(sqrt(g3) * 65536.0))
 *     with the correctly rounded f64 square root and rounding to nearest even.  0xFFFFFFFF: there is no feature.
 *   Per image and measured value: A the image's set and S_A its surface voxels, B the reference's set and S_B its surface
 *     voxels, D_B the transform with F = S_B and D_A the one with F = S_A.
 *       n_a = |S_A|;  n_b = |S_B|
 *       sum_ab = sum over v in S_A of D_B[v];  sum_ba = sum over v in S_B of D_A[v]                       (u64)
 *       max_ab, max_ba: the largest of those distances                                                    (u32)
 *       pct_ab = the k-th smallest of {D_B[v] : v in S_A}, k = (p * n_a + 99) / 100 (1-based, integer division); pct_ba likewise
 *       with D_A, S_B and n_b.  p = 100 is the maximum.
 *     If n_a == 0 or n_b == 0 both sums are 0 and the four distances are 0xFFFFFFFF.
 *   What users read is formed from the row on the host, here and nowhere else:
 *       hausdorff   = (double)max(max_ab, max_ba) * 2^-16
 *       hausdorff_p = (double)max(pct_ab, pct_ba) * 2^-16
 *       assd        = ((double)(sum_ab + sum_ba) / (double)(n_a + n_b)) * 2^-16
 *     all three NaN when n_a == 0 or n_b == 0.
 * Device memory of an accumulator on V voxels with n measured values: 4 n V bytes (one map D_B per value), 6 V bytes (the
 * reference's and the current image's dense label index and surface mask), two f64 planes of the largest bounding box of an
 * image's and the reference's set of one value (at most 16 V bytes), 8 bytes per surface voxel of the image and the reference,
 * and the staging of one source volume and of its resliced copy.
 * FROG_E_INVALID, before the device is touched: a NULL argument, a float volume, an empty grid or one above 2^31 voxels, a
 * spacing that is not positive and finite, n_values == 0 or > FROG_SURFACE_MAX_LABELS, values that are not strictly ascending,
 * a percentile outside 1..100, a mode other than 0 or 1; in add a background that is not finite, a chain on another device, a
 * source without a chain whose dims differ from the grid's.  A refused device allocation is FROG_E_NOMEM: a failed create leaves
 * nothing allocated, a failed add leaves the accumulator as it was. */
#define FROG_SURFACE_MAX_LABELS 256
/* out[v] = the stored distance from voxel v to the set {labels == value} (mode 0) or to that set's surface voxels (mode 1), at
 * labels->spacing.  `labels` has one of the six integer types; host arrays, out has one uint32 per voxel, x fastest. */
int  frog_distance_map(const frog_volume *labels, int64_t value, int mode, int device, uint32_t *out);

typedef struct frog_surface_row {
    uint64_t n_a, n_b, sum_ab, sum_ba;
    uint32_t max_ab, max_ba, pct_ab, pct_ba;
} frog_surface_row;
typedef struct frog_surface frog_surface;
/* `reference`: an integer label volume with host data; its dims, origin and spacing are the grid.  `values`: the n_values
 * measured label values, strictly ascending (signed).  The maps D_B of all values are computed here. */
int  frog_surface_create(const frog_volume *reference, const int64_t *values, uint32_t n_values, uint32_t percentile,
                         int device, frog_surface **out);
/* One image against the reference.  The image's label at a grid voxel is taken exactly as frog_labels_add takes it: with a
 * chain the voxel frog_chain_reslice(chain, source, out, 0, background) stores there (the same device code), with
 * chain == NULL the source's own voxel (its dims must equal the grid's).  A label of the image that is not in `values` is
 * measured nowhere; it still ends its neighbours' sets, so it makes surface.  rows[j] is the row of values[j].  The call keeps
 * nothing of the image: adds are independent of each other and of their order. */
int  frog_surface_add(frog_surface *a, frog_chain *chain, const frog_volume *source, double background, frog_surface_row *rows);
void frog_surface_destroy(frog_surface *a);

/* ---- a per-voxel linear model over the group and its permutation test (an extension: tensor-based morphometry; the reference
 * has no counterpart) ------------------------------------------------------------------------------------------------------------
 * Where do the images of a registered group differ from each other: per grid voxel the model y_i = sum_j X_ij beta_j + e_i over
 * the images i that take part there, y_i the image's value (its resliced intensity, or the Jacobian determinant of its chain or
 * its logarithm), X the n_images x n_columns design (row i belongs to add number i), one t statistic per contrast, and the
 * maximum and minimum of each t over the voxels under permutations of the design, from which family-wise corrected p-values are
 * formed (Nichols and Holmes, Human Brain Mapping 15, 2002).
 * The accumulator holds the z-planes [first_plane, first_plane + n_planes) of `grid`, the WINDOW, exactly as frog_rank does: a
 * voxel's position is computed from its index in the whole grid, so windows that partition the grid give, bit for bit, what one
 * whole-grid window gives.  The device holds one f32 per image and window voxel; the bits 0x7FC00000 (a NaN) mean "does not take
 * part".  frog_glm_planes is frog_rank_planes.
 *
 * What an add keeps.  Add number i fills plane i of the window.
 *   frog_glm_add: x and the voxel's validity exactly as frog_rank_add takes them; the entry takes part iff the voxel is valid
 *     and x is finite.
 *   frog_glm_add_jacobian: det is the f64 value frog_chain_sample(chain, grid ...) stores for that node (the same device code).
 *     The voxel is valid iff its position after the chain passes frog_cover_add's inside test against `support` (a frog_volume
 *     of which only dims, origin and spacing are read; NULL: valid everywhere) and then frog_cover_add's mask rule at the same
 *     position (mask may be NULL).  The chain is evaluated once.  log_mode 0: x = (float)det.  log_mode 1: x = (float)log(det)
 *     where det > 0; elsewhere the entry does not take part, so a folded voxel is excluded.  The device's f64 log is not
 *     correctly rounded (1 ulp, HIP's math table): that line alone is not stated to the bit.  Everything below is stated on the
 *     stored plane, which frog_glm_plane returns.  A chain is required.
 *   frog_glm_plane: what add number image_index stored, window-sized, 0x7FC00000 where the entry does not take part.
 *
 * frog_glm_finish and frog_glm_permute require exactly n_images adds.  Per window voxel, every floating-point line below is one
 * separately rounded f64 operation (no contraction), loops ascending unless said otherwise.  p = n_columns.
 *   Design rows X'.  In finish X'_i = X_i.  In permutation k of permute, for the columns j whose bit is set in `columns`:
 *       X'_ij = (double)sign[k][i] * X[perm[k][i]][j]                     (one multiplication; sign == NULL: 1.0)
 *     and X'_ij = X_ij for every other column (Draper-Stoneman; with all bits set the rows move: Manly; with perm the identity
 *     it is sign flipping, the one-sample test).  perm and sign are n_perms x n_images, row k permutation k.
 *   Participating set.  S = the images whose entry takes part, in add order; k = |S|.  The voxel is UNFIT if `region` (u8,
 *     window-sized, may be NULL) is 0 there or k < max(min_count, p + 1).
 *   Normal equations, over S in add order, each sum from +0.0:
 *       for c <= r:  m = X'_ir * X'_ic;  A_rc = A_rc + m
 *       y = (double)value_i;  for r:  m = X'_ir * y;  b_r = b_r + m
 *   LDL^T with frog_jlabels_finish's loops:
 *       for j:    D_j = A_jj;  for k < j:  q = L_jk * L_jk;  m = q * D_k;  D_j = D_j - m
 *                 for i > j:   x = A_ij;  for k < j:  q = L_ik * L_jk;  m = q * D_k;  x = x - m;   then  L_ij = x / D_j
 *       forward:  z_i = b_i;  for k < i:  m = L_ik * z_k;  z_i = z_i - m
 *       diagonal: y_i = z_i / D_i
 *       backward, i descending:  beta_i = y_i;  for k > i ascending:  m = L_ki * beta_k;  beta_i = beta_i - m
 *     The voxel is UNFIT unless for every j  A_jj > 0  and  D_j > lim_j,  lim_j = 2^-40 * A_jj: a covering set that leaves one
 *     group empty, or has fewer distinct covariate values than columns, drops out instead of dividing by rounding noise.
 *   Residuals, over S in add order, rss from +0.0:
 *       f = +0.0;  for j:  m = X'_ij * beta_j;  f = f + m;      r = y - f;  q = r * r;  rss = rss + q
 *       s2 = rss / (double)(k - p);  sd = sqrt(s2)                                                  correctly rounded
 *   Per contrast c (p doubles, row c of `contrasts`):  u = the solution of A u = c with the same factor and the same three loops;
 *       v = +0.0;  for j:  m = c_j * u_j;  v = v + m;        e = +0.0;  for j:  m = c_j * beta_j;  e = e + m
 *       den = s2 * v;  den = sqrt(den);  g = e / den;  t = (float)g
 *     Where sd <= sigma_floor (the default 0 catches an exact fit) or t is not finite (a NaN, or a quotient beyond f32):
 *     t = 0x7FC00000.  So t is finite or that one NaN, never +-inf.
 *   finish, window-sized host buffers, any may be NULL, not all: beta (p planes, (float)beta_j), sigma ((float)sd), t (n_contrasts
 *     planes; NULL or n_contrasts == 0: none), count (k, always the raw count).  Unfit voxels get `fill` in beta, sigma and t.
 *   permute: max_t[k * n_contrasts + c] and min_t[...] (either may be NULL, not both) are the largest and smallest t of contrast c
 *     over the window's voxels that are fit under permutation k and whose t is not the NaN; -inf and +inf where there is none.  A
 *     voxel may be fit under one permutation and unfit under another.  The order of floats used is that of frog_rank's keys
 *     (-0 < +0).  Extrema are exact: the result does not depend on scheduling, on how n_perms is cut into calls or launches, or
 *     on windows (combine windows with max and min).  No floating-point atomic is used.
 *
 * frog_glm_draw (host code, no device): permutations and signs from splitmix64,
 *       next():  s += 0x9E3779B97F4A7C15;  z = s;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *                return z ^ z >> 31                                              (u64 arithmetic; s starts at seed)
 *   Row 0 is the identity with every sign +1 and consumes no draw.  For k >= 1 in turn: perm[k] starts as the identity; with
 *   shuffle != 0, for i = n - 1 down to 1:  j = next() % (i + 1);  swap perm[k][i] and perm[k][j]  (Fisher-Yates; the modulo bias
 *   is below n / 2^64 < 2^-52); then with flip != 0, for i ascending:  sign[k][i] = (next() >> 63) ? -1 : +1;  without flip +1.
 *   sign may be NULL when flip == 0.
 *
 * FROG_E_INVALID, before the device is touched: a NULL argument that is not marked optional, everything frog_rank_create refuses
 * for the grid and the window, n_images == 0 or > FROG_GLM_MAX_IMAGES, n_columns == 0 or > FROG_GLM_MAX_COLUMNS,
 * n_images <= n_columns, a design entry that is not finite; in the adds what frog_rank_add refuses, a NULL chain or a support
 * or mask the chain cannot sample in add_jacobian, the (n_images + 1)th add; in plane an image_index not yet added; in finish
 * and permute fewer than n_images adds, min_count == 0, n_contrasts > FROG_GLM_MAX_CONTRASTS, a contrast entry that is not
 * finite, a sigma_floor that is negative or NaN, no output; in permute n_contrasts == 0, n_perms == 0, a perm entry >= n_images,
 * a sign other than +-1, columns == 0 or with a bit >= n_columns; in draw n == 0 or > FROG_GLM_MAX_IMAGES, n_perms == 0. */
#define FROG_GLM_MAX_IMAGES 4096
#define FROG_GLM_MAX_COLUMNS 8
#define FROG_GLM_MAX_CONTRASTS 8
typedef struct frog_glm frog_glm;
int  frog_glm_planes(const frog_volume *grid, uint32_t n_images, int device, uint32_t *planes);
int  frog_glm_create(const frog_volume *grid, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, uint32_t n_columns,
                     const double *design, int device, frog_glm **out);
int  frog_glm_add(frog_glm *a, frog_chain *chain, const frog_volume *source, const frog_volume *mask, int interpolation, double background);
int  frog_glm_add_jacobian(frog_glm *a, frog_chain *chain, const frog_volume *support, const frog_volume *mask, int log_mode);
int  frog_glm_plane(frog_glm *a, uint32_t image_index, float *values);
int  frog_glm_finish(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                     const uint8_t *region, float fill, float *beta, float *sigma, float *t, uint16_t *count);
int  frog_glm_permute(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                      const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign,
                      float *max_t, float *min_t);
int  frog_glm_draw(uint32_t n, uint32_t n_perms, uint64_t seed, int shuffle, int flip, uint32_t *perm, int8_t *sign);
void frog_glm_destroy(frog_glm *a);

/* ---- connected components and the cluster-extent test (an extension; the reference has no counterpart) --------------------------
 * A MASK is a set of voxels of a 3-D grid, x fastest.  Two set voxels are neighbours at connectivity 6 when they share a face
 * (|dx| + |dy| + |dz| == 1), at 18 when they share a face or an edge (max(|dx|, |dy|, |dz|) == 1 and the sum <= 2), at 26 when
 * max(|dx|, |dy|, |dz|) == 1; a COMPONENT is a class of the transitive closure.  The last voxel of a row and the first of the
 * next are no neighbours: adjacency is of coordinates, not of indices.
 *   root(v)   = the smallest linear index x + nx * (y + ny * z) of v's component
 *   extent    = the number of voxels of a component
 *   label(v)  = 1 + #{roots below root(v)} at a set voxel, 0 elsewhere: 1..K in ascending order of root
 * Every result is an integer and exact: it does not depend on scheduling (integer atomic minimum, sum and maximum only).
 *
 * frog_components: the mask is the non-zero voxels of an integer volume with host data.  labels (u32, grid-sized),
 * n_components (K) and largest (the largest extent, 0 for an empty mask) may each be NULL, not all.
 *
 * frog_clusters, the SINK of a permutation test: on the device, for the whole grid, one bit mask per SLOT (permutation,
 * contrast, side), slot = (perm * n_contrasts + contrast) * sides + side, sides = 2 with two_sided and 1 without, all empty
 * at first.  Side 0 is the positive side, side 1 the negative.
 *   frog_glm_permute_clusters does what frog_glm_permute does with the same arguments; max_t and min_t (either or both may be
 *     NULL here) are bit for bit frog_glm_permute's.  For row k of the call and contrast c it also sets, in the slots of
 *     permutation first_perm + k, the bit of every window voxel at the voxel's index in the whole grid, where the voxel is
 *     fit under that permutation and its t is not the NaN -- the voxels the extrema are taken over -- and
 *         side 0:  t > threshold            side 1:  t < -threshold          (f32 comparisons on that t)
 *     Windows that partition the grid fill one mask between them, so a cluster that crosses a window boundary is one
 *     cluster.  The sink counts the z-planes each permutation has received: a plane written twice is FROG_E_STATE (nothing
 *     is computed then).
 *   frog_clusters_finish: max_extent[slot] = the largest extent of the slot's mask at the sink's connectivity, 0 for an empty
 *     mask.  FROG_E_STATE unless every permutation has received every plane of the grid.
 *   frog_clusters_mask: one slot as bytes (0 or 1), grid-sized.
 *   frog_clusters_labels: one slot's labels as frog_components gives them (n_components may be NULL).  FROG_E_STATE unless the
 *     permutation has received every plane.
 * Device memory: slots * ceil(voxels / 32) words for the masks, and 8 bytes per voxel for each of the masks that are labelled
 * in one launch (at most 64, fewer where memory is short).  FROG_E_NOMEM, with the bytes needed and the bytes free in the
 * message, when the masks and the workspace of one mask do not fit.
 *
 * FROG_E_INVALID, before the device is touched: a NULL argument that is not marked optional, a grid that is empty or above 2^31
 * voxels, a connectivity other than 6, 18 or 26, a threshold that is negative or not finite, n_perms == 0, n_contrasts == 0 or
 * > FROG_GLM_MAX_CONTRASTS, a float mask volume or one without data, everything frog_glm_permute refuses, a sink whose grid
 * dims, device or n_contrasts differ from the accumulator's and the call's, first_perm + n_perms beyond the sink's n_perms,
 * a permutation, contrast or side that the sink does not have. */
int  frog_components(const frog_volume *mask, int connectivity, int device, uint32_t *labels, uint32_t *n_components, uint64_t *largest);

typedef struct frog_clusters frog_clusters;
int  frog_clusters_create(const frog_volume *grid, uint32_t n_perms, uint32_t n_contrasts, int two_sided, float threshold,
                          int connectivity, int device, frog_clusters **out);
int  frog_glm_permute_clusters(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                               const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign,
                               uint32_t first_perm, frog_clusters *sink, float *max_t, float *min_t);
int  frog_clusters_finish(frog_clusters *s, uint32_t *max_extent);
int  frog_clusters_mask(frog_clusters *s, uint32_t perm, uint32_t contrast, int side, uint8_t *mask);
int  frog_clusters_labels(frog_clusters *s, uint32_t perm, uint32_t contrast, int side, uint32_t *labels, uint32_t *n_components);
void frog_clusters_destroy(frog_clusters *s);

/* ---- threshold-free cluster enhancement, TFCE (an extension; Smith and Nichols, NeuroImage 44, 2009) ---------------------------
 * Parameters: dh (f32, finite, > 0), E (0.5 or 1), H (1 or 2), connectivity (6, 18 or 26).  Components and extents are those
 * of the section above.
 *
 * LEVEL of a statistic t (f32) on a side:
 *   s = t on side 0, s = -t on side 1
 *   L = 0                                         where t is the NaN or s <= 0
 *   q = (double)s / (double)dh                    one f64 division, correctly rounded
 *   L = q >= 255 ? 255 : (uint8_t)q               truncation; a statistic beyond 255 * dh SATURATES at level 255
 *
 * ENHANCEMENT of a level map:
 *   M_k    = { v : L(v) >= k },  e_k(v) = the extent of v's component of M_k
 *   h_k    = (double)k * (double)dh
 *   w_k    = (H == 2 ? h_k * h_k : h_k) * (double)dh          separately rounded f64 products
 *   g(e)   = E == 0.5 ? sqrt((double)e) : (double)e            the correctly rounded f64 square root
 *   acc    = +0.0;  for k = L(v) down to 1:  m = g(e_k(v)) * w_k;  acc = acc + m       (f64, in this order, no FMA)
 *   tfce(v) = (float)acc, which is 0 where L(v) == 0
 * No floating-point atomic is used: a voxel's sum is its own, and a maximum over voxels is an integer maximum on the bits of
 * non-negative f32 values.  Every result is the same from run to run.
 *
 * frog_tfce_volume: the enhancement of one side (0 or 1) of any FROG_V_F32 volume with host data; tfce (f32, grid-sized) and
 * max (the largest tfce, 0 where every level is 0) may each be NULL, not both.
 *
 * frog_tfce, the SINK of a permutation test: on the device, for the whole grid, one u8 level per voxel and SLOT,
 * slot = (perm * n_contrasts + contrast) * sides + side as for frog_clusters, all zero at first.
 *   frog_glm_permute_tfce does what frog_glm_permute does with the same arguments; max_t and min_t (either or both may be NULL
 *     here) are bit for bit frog_glm_permute's.  For row k of the call and contrast c it also stores, in the slots of
 *     permutation first_perm + k, at the voxel's index in the whole grid, the level of every window voxel that is fit under
 *     that permutation and whose t is not the NaN -- the voxels the extrema are taken over -- and 0 for the window's other
 *     voxels.  Windows that partition the grid fill one level map between them.  The sink counts the z-planes each
 *     permutation has received: a plane written twice is FROG_E_STATE (nothing is computed or written then).
 *   frog_tfce_finish: max_tfce[slot] = the largest tfce(v) of the slot, 0 for a slot without a positive level.  FROG_E_STATE
 *     unless every permutation has received every plane of the grid.
 *   frog_tfce_levels: one slot's levels, grid-sized.
 *   frog_tfce_map: one slot's tfce, grid-sized.  FROG_E_STATE unless the permutation has received every plane.
 * Device memory: slots * (voxels rounded up to a multiple of 32) bytes for the levels, and 16 bytes per voxel plus a bit mask
 * for each of the slots that are enhanced in one launch (at most 64, fewer where memory is short).  FROG_E_NOMEM, with the
 * bytes needed and the bytes free in the message, when the levels and the workspace of one slot do not fit.
 *
 * FROG_E_INVALID, before the device is touched: a NULL argument that is not marked optional, a grid that is empty or above 2^31
 * voxels, dh that is not finite or not above 0, E other than 0.5 or 1, H other than 1 or 2, a connectivity other than 6, 18 or
 * 26, n_perms == 0, n_contrasts == 0 or > FROG_GLM_MAX_CONTRASTS, a side other than 0 or 1, a volume that is not FROG_V_F32 or
 * has no data, everything frog_glm_permute refuses, a sink whose grid dims, device or n_contrasts differ from the
 * accumulator's and the call's, first_perm + n_perms beyond the sink's n_perms, a permutation, contrast or side that the sink
 * does not have. */
int  frog_tfce_volume(const frog_volume *stat, int side, float dh, double E, double H, int connectivity, int device, float *tfce, float *max);

typedef struct frog_tfce frog_tfce;
int  frog_tfce_create(const frog_volume *grid, uint32_t n_perms, uint32_t n_contrasts, int two_sided, float dh, double E, double H,
                      int connectivity, int device, frog_tfce **out);
int  frog_glm_permute_tfce(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                           const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign,
                           uint32_t first_perm, frog_tfce *sink, float *max_t, float *min_t);
int  frog_tfce_finish(frog_tfce *s, float *max_tfce);
int  frog_tfce_levels(frog_tfce *s, uint32_t perm, uint32_t contrast, int side, uint8_t *levels);
int  frog_tfce_map(frog_tfce *s, uint32_t perm, uint32_t contrast, int side, float *tfce);
void frog_tfce_destroy(frog_tfce *s);

/* ---- smoothing the maps before the fit: a coverage-aware Gaussian (an extension; the reference has no counterpart) --------------
 * A normalised convolution over the voxels that take part (Knutsson and Westin, CVPR 1993): the background of an image's field
 * of view is not pulled into its rim, and the set of voxels that take part does not change.  sigma is in mm and isotropic; each
 * axis has its own spacing, so the radii and the taps differ per axis.  fwhm = FROG_SMOOTH_FWHM * sigma.
 *
 * frog_smooth_taps (host code, no device): the radius and the taps w_0 .. w_R of one axis with spacing s.  Every line is one
 * rounded f64 operation, exp is the host libm's:
 *       q = 3.0 * sigma;  q = q / s;  R = (uint32_t)ceil(q)
 *       den = 2.0 * sigma;  den = den * sigma
 *       for d = 0 .. R:  x = (double)d * s;  x = x * x;  x = x / den;  w_d = exp(-x)
 *   w_0 is exactly 1: the quotient below normalises, not the taps.  taps (FROG_SMOOTH_MAX_RADIUS + 1 doubles, of which R + 1 are
 *   written) may be NULL.  The taps are DATA: the device code uses exactly the doubles this function returns, uploaded as they
 *   are, so nothing below depends on any exp being correctly rounded.
 *
 * A SMOOTHED VOLUME, of f32 values x with a per-voxel "takes part".  Two f64 fields start per voxel as
 *       num = takes part ? (double)x : +0.0          den = takes part ? 1.0 : +0.0
 *   Three passes follow, along x, then y, then z, each applied to both fields with the axis's R and taps.  Per voxel v and field:
 *       acc = +0.0;  for d = -R .. +R ascending:  m = w_|d| * in(v + d * e_axis);  acc = acc + m
 *   where a neighbour outside the grid contributes the term +0.0.  Every line is one rounded f64 operation, no contraction; a
 *   pass reads the f64 values the pass before it gave, never rounded to f32.  No sum is ever -0.0 (it starts from +0.0, and
 *   round-to-nearest gives +0.0 for x + (-x)), so a term of +0.0 changes no bit: the sums carry the bits of the loop over the
 *   neighbours inside the grid alone, and a voxel that does not take part counts exactly as one outside the grid.
 *       result = (float)(num / den)     where the voxel itself takes part: one correctly rounded division; den >= 1 there,
 *                                       because w_0 == 1 and every term is >= +0.0
 *       result = 0x7FC00000             where it does not
 *   Smoothing never changes which voxels take part: counts and coverage stay as they are.  A voxel that takes part and has no
 *   participating neighbour within the radii keeps its value exactly (num = x, den = 1; a -0.0 comes back as +0.0).  No floating-point atomic is used and
 *   no result depends on scheduling, on how a launch is cut, or on windows.
 *
 * frog_smooth_volume: any FROG_V_F32 volume with host data, smoothed on `device` with the volume's own spacing; out is f32,
 *   grid-sized.  take (u8, grid-sized) may be NULL: then a voxel takes part iff its value is finite; with take iff its flag is
 *   non-zero and its value is finite.  sigma_mm == 0: every radius is 0, so a voxel that takes part keeps its value.
 *
 * frog_glm_smooth: legal only before the first add (FROG_E_STATE after one); sigma_mm == 0 turns smoothing off, which is how an
 *   accumulator starts.  Afterwards every frog_glm_add and frog_glm_add_jacobian stores the smoothed value in place of the raw
 *   one: the RAW MAP of add i is what the same call without smoothing would store at every voxel of the WHOLE grid, a voxel
 *   takes part iff its raw entry is not 0x7FC00000, the map is smoothed as above with the grid's spacing, and the window's part
 *   is kept.  So windows that partition the grid still give, bit for bit, what one whole-grid window gives, and everything
 *   stated on the stored plane above -- frog_glm_plane, finish, the three permute calls and their sinks -- holds as it stands.
 *   The add evaluates the raw map on the window extended by R_z planes on each side, clipped at the grid's ends, with the same
 *   device code on a larger range: a halo costs extra evaluations only where the grid is cut into windows.
 *   Device memory: 36 bytes per voxel of that extended range, allocated by frog_glm_smooth.  FROG_E_NOMEM, with the bytes needed
 *   and the bytes free in the message, when it does not fit; the accumulator then stays unsmoothed.
 * frog_glm_smooth_planes: frog_glm_planes with the scratch of the halo counted: the most planes p such that the n_images planes
 *   of p z-planes and 36 bytes per voxel of min(p + 2 R_z, dims[2]) planes fit half of the free device memory; sigma_mm == 0
 *   gives frog_glm_planes' answer.
 *
 * FROG_E_INVALID, before the device is touched: a NULL argument that is not marked optional, a sigma that is negative or not
 * finite (in frog_smooth_taps also 0), a spacing that is not finite or not above 0, a radius above
 * FROG_SMOOTH_MAX_RADIUS along any axis, a volume that is not FROG_V_F32, has no data, is empty or above 2^31 voxels,
 * everything frog_glm_planes refuses. */
#define FROG_SMOOTH_MAX_RADIUS 64
#define FROG_SMOOTH_FWHM 2.3548200450309493         /* 2 sqrt(2 ln 2): sigma = fwhm / FROG_SMOOTH_FWHM */
int  frog_smooth_taps(double sigma_mm, double spacing, uint32_t *radius, double *taps);
int  frog_smooth_volume(const frog_volume *volume, const uint8_t *take, double sigma_mm, int device, float *out);
int  frog_glm_smooth(frog_glm *a, double sigma_mm);
int  frog_glm_smooth_planes(const frog_volume *grid, uint32_t n_images, double sigma_mm, int device, uint32_t *planes);

/* ---- principal modes of a registered group: a statistical deformation model (an extension; Rueckert, Frangi and Schnabel, IEEE
 * TMI 22(8), 2003: a principal component analysis of the images' deformation fields in the group's space) ----------------------
 * How does the group vary as a whole: the mean of the images' values, a few modes (each a field of values per standard
 * deviation), the share of the variance each explains, and per image a score on every mode.  A value is the displacement of the
 * image's chain in mm (3 components), or one of frog_glm's three scalar kinds (1 component).
 * The accumulator holds the z-planes [first_plane, first_plane + n_planes) of `grid`, the WINDOW, exactly as frog_glm does, and
 * n_components (1 or 3) f32 per image and window voxel, component fastest; the bits 0x7FC00000 mean "does not take part".
 * frog_modes_planes is frog_rank_planes' rule for n_images * n_components values per voxel.
 *
 * What an add keeps.  Add number i fills entry i of the window.
 *   frog_modes_add_displacement (3 components): d is the f64 displacement frog_chain_sample(chain, grid ...) stores for that node
 *     (the same device code), x_k = (float)d_k.  The voxel is valid exactly as in frog_glm_add_jacobian (support, then mask, at
 *     the position the same evaluation of the chain gives); it takes part iff it is valid and all three x_k are finite, else all
 *     three entries are 0x7FC00000.  A chain is required.
 *   frog_modes_add_jacobian and frog_modes_add (1 component): bit for bit what frog_glm_add_jacobian and frog_glm_add store (the
 *     same kernels).  There is no smoothing here.
 *   frog_modes_plane: what add number image_index stored, window-sized, n_components floats per voxel.  Everything below is stated
 *     on these planes.
 *
 * Every floating-point line below is one separately rounded f64 operation (no contraction), loops ascending.  n = n_images, x_i
 * the stored f32 of image i at one voxel and component.
 *   SUPPORT.  A window voxel is in the support iff `region` (u8, window-sized, may be NULL) is non-zero there and every image
 *     takes part there: a principal component analysis needs complete rows.
 *   Mean and centring, per support voxel and component:
 *       s = +0.0;  for i:  s = s + (double)x_i;      m = s / (double)n;      c_i = (double)x_i - m
 *     Outside the support c_i = +0.0 for every i.
 *
 * frog_modes_gram: gram is the packed lower triangle, entry (i, j), j <= i, at i (i + 1) / 2 + j, n (n + 1) / 2 doubles.  It is
 *   READ AND UPDATED, and so is n_support (the number of support voxels is added to it).
 *   The values of one z-plane in index order (x fastest, then y, component fastest of all) are cut into CHUNKS of FROG_MODES_CHUNK
 *   consecutive values; the last chunk of a plane may be shorter.  Per pair j <= i:
 *       chunk:   s = +0.0;  for the chunk's values ascending:  p = c_i * c_j;  s = s + p
 *       plane:   t = +0.0;  for the plane's chunks ascending:  t = t + s_chunk
 *       window:  for the window's planes ascending:  gram_ij = gram_ij + t_plane
 *   So windows that partition the grid, taken in ASCENDING plane order with gram passed on from one to the next, give the bits of
 *   one whole-grid window.  THE ORDER OF THE WINDOWS MATTERS HERE, and here only: every other result of this library is
 *   independent of the order its windows are taken in.  No floating-point atomic is used, and no sum depends on scheduling.
 *
 * frog_modes_project: weights is n_modes x n_images, row k the weights w_k of mode k.  Per support voxel and component
 *       mean = (float)m
 *       mode_k:  s = +0.0;  for i:  p = w_ki * c_i;  s = s + p;      mode_k = (float)s
 *   and `fill` outside the support.  mean (window-sized, n_components floats per voxel; may be NULL) and modes (n_modes such
 *   fields, mode k first) are host buffers.  Windows are independent.
 *
 * frog_modes_eigen (host code, no device): the eigen-decomposition of the symmetric matrix G = gram / divisor (gram packed as
 *   above, one division per entry) by the cyclic Jacobi method in f64.
 *       d = the largest |G_ij|;  tol = 2^-60 * d
 *       a SWEEP visits the pairs (p, q), p < q, p ascending and for each p q ascending.  A pair with |G_pq| <= tol is left as it
 *       is.  Every other pair is ROTATED:
 *           theta = (G_qq - G_pp) / (2 G_pq);  t = sgn(theta) / (|theta| + sqrt(theta^2 + 1))   (sgn(0) = +1)
 *           c = 1 / sqrt(t^2 + 1);  s = t c
 *           G_pp = G_pp - t G_pq;  G_qq = G_qq + t G_pq;  G_pq = G_qp = 0
 *           for k other than p, q:  G_kp' = c G_kp - s G_kq;  G_kq' = s G_kp + c G_kq      (and their mirror images)
 *           for k:                  E_kp' = c E_kp - s E_kq;  E_kq' = s E_kp + c E_kq      (E starts as the identity)
 *       Sweeps are repeated until one rotates nothing.  The eigenvalues are then the diagonal, the eigenvectors the columns of E.
 *   values[k] descend; ties keep index order (a stable sort).  vectors is n x n, row k the eigenvector of values[k]: unit length
 *   (it is renormalised once at the end), and its entry of largest magnitude (the lowest index on ties) is positive.
 *   What users read is formed from these on the host: with divisor = n - 1, weights w_ki = vectors[k][i] / sqrt(n - 1) give
 *   modes per standard deviation, and b_ik = sqrt(n - 1) * vectors[k][i] is image i's score on mode k in standard deviations.
 *
 * Device memory: 4 * n_images * n_components bytes per window voxel, allocated by create; gram and project work through the
 * window in batches whose scratch stays below 256 MiB (or one z-plane's, where that is more).
 * Left out: voxels that some image does not cover (they are outside the support), more than FROG_MODES_MAX_IMAGES images,
 * log-Euclidean and velocity-field statistics, leave-one-out generalisation and specificity.
 *
 * FROG_E_INVALID, before the device is touched: a NULL argument that is not marked optional, everything frog_glm_create refuses
 * for the grid and the window, n_images < 2 or > FROG_MODES_MAX_IMAGES, n_components other than 1 or 3; in the adds what the
 * frog_glm adds refuse, an add whose kind does not fit n_components, the (n_images + 1)th add; in plane an image_index not yet
 * added; in gram and project fewer than n_images adds; in project n_modes == 0 or > n_images, a weight that is not finite; in
 * eigen n == 0 or > FROG_MODES_MAX_IMAGES, a divisor that is not > 0 (or not finite), a gram entry that is not finite. */
#define FROG_MODES_MAX_IMAGES 512
#define FROG_MODES_CHUNK 1024
typedef struct frog_modes frog_modes;
int  frog_modes_planes(const frog_volume *grid, uint32_t n_images, uint32_t n_components, int device, uint32_t *planes);
int  frog_modes_create(const frog_volume *grid, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, uint32_t n_components,
                       int device, frog_modes **out);
int  frog_modes_add_displacement(frog_modes *a, frog_chain *chain, const frog_volume *support, const frog_volume *mask);
int  frog_modes_add_jacobian(frog_modes *a, frog_chain *chain, const frog_volume *support, const frog_volume *mask, int log_mode);
int  frog_modes_add(frog_modes *a, frog_chain *chain, const frog_volume *source, const frog_volume *mask, int interpolation, double background);
int  frog_modes_plane(frog_modes *a, uint32_t image_index, float *values);
int  frog_modes_gram(frog_modes *a, const uint8_t *region, double *gram, uint64_t *n_support);
int  frog_modes_project(frog_modes *a, const uint8_t *region, uint32_t n_modes, const double *weights, float fill, float *mean, float *modes);
int  frog_modes_eigen(uint32_t n, const double *gram, double divisor, double *values, double *vectors);
void frog_modes_destroy(frog_modes *a);

/* ---- iso-surfaces: a welded triangle mesh from a scalar volume at a level, or from a label map at a value (an extension; the
 * reference has tools/MeshTransform.cxx for meshes made elsewhere, and nothing that makes one) ---------------------------------
 * Marching tetrahedra on the Kuhn (Freudenthal) decomposition of every grid cell: translation invariant and face compatible,
 * so neighbouring cells agree without a parity rule and the mesh is a closed 2-manifold wherever the surface does not touch the
 * grid's border.  No hashing and no atomics: the output is the same bytes from run to run.
 *   Nodes.  The voxels of `volume` (any FROG_V_* type), node (i, j, k) at origin + (i, j, k) * spacing in f64 per axis, as
 *     frog_chain_sample forms it; node index = i + dims[0] * (j + dims[1] * k).
 *   Inside. FROG_ISO_LEVEL: iff (double)v >= level (a NaN voxel is outside).  FROG_ISO_LABEL: iff the voxel as a signed 64-bit
 *     integer equals `value`; integer types only.
 *   Cells.  A cell belongs to its lowest node.  Its six tetrahedra are taken in the lexicographic order of the permutations pi
 *     of the axes: xyz, xzy, yxz, yzx, zxy, zyx.  Tetrahedron pi has the vertices v0 = (0,0,0), v1 = v0 + e_pi0,
 *     v2 = v1 + e_pi1, v3 = (1,1,1) of the cell.
 *   Triangles of a tetrahedron, by its inside set; a triangle vertex is named by the tetrahedron edge it lies on, a pair of
 *     tetrahedron vertex numbers:
 *       0 or 4 inside                                  none
 *       1 inside, a; the others b < c < d              (ab, ac, ad)
 *       3 inside, b < c < d; a outside                 (ba, ca, da)
 *       2 inside, a < b; c < d outside                 the quad (ac, ad, bd, bc) cut as (ac, ad, bd) and (ac, bd, bc)
 *   Orientation.  With the triangle's vertices at the edges' midpoints in the unit cube: if normal . (mean of the outside
 *     corners - mean of the inside corners) <= 0, its second and third vertices are swapped.  The product is never 0.  Normals
 *     point from inside to outside; the first vertex never moves.
 *   Vertices.  One per crossing edge (its ends differ in the inside test).  An edge belongs to its lower node, which owns seven:
 *     (dx, dy, dz) != 0 with code dx + 2 dy + 4 dz - 1 -- three axis edges, three face diagonals, the body diagonal.  For the
 *     owner a and the other end b, in f64:
 *       FROG_ISO_LEVEL: t = (level - va) / (vb - va); t = 0.5 if va or vb is not finite.      FROG_ISO_LABEL: t = 0.5.
 *       per axis p = pa + t * (pb - pa), stored as one (float) cast.
 *     A voxel equal to the level gives t = 0 or 1; the degenerate triangles this makes are kept (dropping them opens the mesh).
 *   Order, part of the interface.  Vertices ascend by owner node index, within a node by edge code.  Triangles ascend by cell
 *     in the same node order, within a cell by tetrahedron, within a tetrahedron in the rule's order.  The vertex on an edge has
 *     the index vertex_offset[owner] + popcount(mask[owner] & ((1 << code) - 1)), mask the owner's 7-bit set of crossing edges
 *     and vertex_offset the exclusive sum of the masks' popcounts over the nodes.
 * A grid with a dimension below 2, or with nothing inside: 0 vertices, 0 triangles, FROG_OK (and a handle).
 * FROG_E_INVALID: a NULL argument; an unknown mode or dtype; a float dtype in label mode; a NaN level; more than 2^31 nodes
 * (all before the device is touched); a result of 2^31 or more vertices or triangles, found from 64-bit totals before
 * anything is allocated for it.
 * Device memory while create runs: the volume, 6 bytes per node and the mesh (12 bytes per vertex and per triangle); the
 * handle keeps the mesh. */
enum { FROG_ISO_LEVEL = 0, FROG_ISO_LABEL = 1 };
typedef struct frog_isosurface frog_isosurface;
int  frog_isosurface_create(const frog_volume *volume, int mode, double level, int64_t value, int device,
                            frog_isosurface **out, uint32_t *n_vertices, uint32_t *n_triangles);
/* vertices <- (float)chain((double)vertex), on the device where they lie: frog_chain_apply_f32 without the copies.  A chain on
 * another device -> FROG_E_INVALID. */
int  frog_isosurface_apply(frog_isosurface *s, frog_chain *chain);
/* n_vertices x 3 floats and n_triangles x 3 indices into host arrays (either may be NULL when its count is 0). */
int  frog_isosurface_get(frog_isosurface *s, float *xyz, uint32_t *triangles);
void frog_isosurface_destroy(frog_isosurface *s);
/* out[i] = (float)chain((double)in[i]), n points of 3 floats (host arrays): frog_chain_apply on the widened points (the same
 * device code), cast once.  What bin/MeshTransform moves a mesh's points with. */
int  frog_chain_apply_f32(frog_chain *c, const float *in3n, float *out3n, size_t n);

/* ---- mesh filters: non-shrinking smoothing and decimation by vertex clustering, on the device (an extension) -----------------
 * A mesh is n points (f32 xyz) and faces given as face_ptr / face_idx (u32), as in frog_mesh (frog_host.h); a frog_isosurface
 * holds triangles, face f = indices 3 f .. 3 f + 2.  No hashing and no atomics: the same bytes from run to run.
 *
 * Edges, neighbours, boundary.
 *   The edges of a face are its cyclic consecutive index pairs (the last index pairs with the first; a face of two indices
 *     gives its pair twice, a face of one index a pair of equal indices).  A pair of two equal indices is ignored.
 *   A boundary edge is an unordered pair {a, b} that occurs exactly once among all faces' edges, in whichever orientation: an
 *     edge shared by three faces, or used twice by duplicated faces, is not a boundary edge.
 *   A boundary vertex is an endpoint of at least one boundary edge.
 *   N(v), v not on the boundary: the distinct w != v that share a face edge with v, in ascending index order.
 *   N(v), v on the boundary: with boundary = 1 only the w for which {v, w} is a boundary edge, ascending (the border slides
 *     along itself); with boundary = 0 N(v) is empty, and the neighbours of v still read it.
 *   A vertex with empty N(v) (no face, only ignored pairs, or a boundary vertex with boundary = 0) never moves: its bytes stay.
 * One pass with factor f (Jacobi: every read is of the previous pass's f32 positions).  Per vertex with N(v) not empty, per axis:
 *     s  = the sum of (double)x_w over N(v) in ascending w, starting from +0
 *     m  = s / (double)|N(v)|
 *     x' = (float)((double)x_v + f * (m - (double)x_v))
 *   every operation rounded on its own, none contracted into a fused multiply-add.  Coordinates that are not finite propagate
 *   as IEEE arithmetic makes them: the same infinities and NaNs in the same places (a NaN's sign and payload are not stated).
 * Smoothing (Taubin 1995): `iterations` times a pass with lambda, then a pass with mu.  iterations = 0, or lambda = mu = 0
 *   (either sign of zero), runs no pass: the points keep their bytes.  lambda = mu > 0 is the plain Laplacian.  Faces are
 *   never touched.  The tools' defaults: 20, 0.5, -0.53.
 *
 * Decimation by vertex clustering (Rossignac and Borrel 1993), triangles only, with a cell size `cell` in the units of the
 * points, a finite double > 0:
 *     lo      = the per-axis minimum of the f32 coordinates
 *     c       = (int64)floor(((double)x - (double)lo) / cell) per axis
 *     n_axis  = max c + 1 per axis (at most 2^21)
 *     key     = (c_z * n_y + c_y) * n_x + c_x, 64 bits
 *   New vertex k is the k-th occupied cell in ascending key order.  Its position per axis is (float)(S / (double)count), S the
 *   sum of its members' (double)x in ascending old index, starting from +0.  cluster_of[v] is the new index of old vertex v.
 *   A triangle whose three new indices are not all distinct is dropped; the others keep their relative order and their
 *   orientation.  Nothing else is removed: coincident triangles and vertices without a face stay.  An empty mesh gives an
 *   empty mesh.
 *   What follows.  Every old vertex and its new vertex lie in one closed cell, so they are at most cell * sqrt(3) apart (plus
 *     the f32 cast).  The map on directed edges commutes with reversal and a dropped triangle contributes a cancelling pair
 *     (a -> b, b -> a) or loops, so the image of a closed oriented mesh still uses every directed edge as often as its reverse.
 *   What does not.  The image need not be a 2-manifold: an edge may be used by more than two triangles, two sheets closer than
 *     a cell merge, triangles may coincide (also with opposite orientation), and a vertex may be left without a face.
 *
 * Limits, refused with FROG_E_INVALID before anything is allocated: smoothing takes at most 2^31 - 1 points and 2^30 - 1 face
 * indices (the adjacency sorts two 64-bit keys per index and the sort's counts are signed 32-bit); clustering and upload take
 * fewer than 2^31 points and fewer than 2^31 triangles.
 * FROG_E_INVALID as well: a NULL argument that is not marked optional; a face index >= n; face_ptr that does not start at 0 or
 * descends; lambda or mu that is not finite; boundary other than 0 or 1; in cluster a cell that is not a finite double > 0, a
 * coordinate that is not finite, more than 2^21 cells on an axis.
 * Device memory while a call runs, beyond the mesh: smoothing 40 bytes per face index and the sort's workspace for the adjacency
 * build, then 16 + 4 |N| bytes per vertex and a second copy of the points (12 bytes per vertex); clustering 40 bytes
 * per vertex, the sort's workspace and the new mesh.  The f64 sum of a cluster is sequential (one thread per cluster, as the stated order is): a cell that swallows the
 * whole mesh costs one thread's walk over all n vertices. */
/* host arrays, polygons of any size; xyz is read and written */
int  frog_mesh_smooth(float *xyz, size_t n_points, const uint32_t *face_ptr, const uint32_t *face_idx, size_t n_faces,
                      uint32_t iterations, double lambda, double mu, int boundary, int device);
/* the same device code on the handle's mesh, where it lies */
int  frog_isosurface_smooth(frog_isosurface *s, uint32_t iterations, double lambda, double mu, int boundary);
/* a device mesh from host arrays: n x 3 floats, m x 3 indices (either may be NULL when its count is 0) */
int  frog_isosurface_upload(const float *xyz, uint32_t n, const uint32_t *triangles, uint32_t m, int device, frog_isosurface **out);
/* replaces the handle's mesh by its clustering; cluster_of (host, the old n entries) is optional.  frog_isosurface_get and
 * frog_isosurface_apply work on the result as before. */
int  frog_isosurface_cluster(frog_isosurface *s, double cell, uint32_t *n_vertices, uint32_t *n_triangles, uint32_t *cluster_of);

#ifdef __cplusplus
}
#endif
#endif
