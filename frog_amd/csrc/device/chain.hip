// chain.hip -- forward evaluation and Jacobian of a FROG transform chain (include/frog_chain.h).
// One thread per point, f64; the links live in device memory in application order.  The lattices
// are small (<= a few 10^4 control points) and every thread of a wavefront reads nearby taps, so
// the coefficient loads are L1/L2 hits; the kernel is f64-ALU work (4^3 taps x 12 products per link).
// A sampled displacement field (FROG_T_FIELD) is a link too: eight node reads and a trilinear blend per point, which is
// what frog_chain_sample collapses a whole chain (Newton inverses included) into.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "frog_chain.h"
#include "dev_buf.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <memory>
#include <type_traits>
#include <string>
#include <vector>

namespace frog { void set_last_error(const std::string &s); }

namespace {

constexpr double INVERSE_TOLERANCE = 1e-3;      // vtkWarpTransform::InverseTolerance default
constexpr int INVERSE_ITERATIONS = 500;         // vtkWarpTransform::InverseIterations default

struct DevLink {
    int type;
    double m[12];                   // linear: 3 rows of 4
    int dims[3];
    double origin[3], spacing[3];
    const float *coeffs;
};

__device__ __forceinline__ void basis(double f, double F[4], double G[4])
{
    F[3] = f * f * f / 6;
    F[0] = (f * f - f) / 2 - F[3] + 1.0 / 6;
    F[2] = f + F[0] - F[3] * 2;
    F[1] = 1 - F[0] - F[2] - F[3];
    G[0] = -(1 - f) * (1 - f) / 2;
    G[1] = 1.5 * f * f - 2 * f;
    G[2] = -1.5 * f * f + f + 0.5;
    G[3] = f * f / 2;
}

// A sampled displacement field (FROG_T_FIELD), forward: q = p + d(p), d the trilinear interpolant of the node values.
// Per axis c = (p - origin) / spacing clamped to [0, dims - 1], cell min(floor(c), dims - 2) (0 where dims == 1), fraction
// c - cell: the last node is the last cell's fraction 1, outside the grid the edge value continues.  The eight nodes are
// widened to f64 and combined in reslice_voxel's order.  J = I + dd/dp of the interpolant inside the cell; the column of an
// axis that was clamped, or has one node, is zero.  A NaN coordinate passes the comparisons and makes q NaN.
template <bool JAC>
__device__ __forceinline__ void field_forward(const DevLink &t, const double p[3], double q[3], double J[3][3])
{
    int i0[3], i1[3];
    double f[3];
    bool flat[3];
    for (int k = 0; k < 3; k++) {
        const int last = t.dims[k] - 1;
        const double raw = (p[k] - t.origin[k]) / t.spacing[k];
        const double c = raw < 0.0 ? 0.0 : (raw > (double)last ? (double)last : raw);
        i0[k] = c < (double)last ? (int)floor(c) : (last > 0 ? last - 1 : 0);      // 0 <= c < last before the int conversion
        i1[k] = last > 0 ? i0[k] + 1 : 0;
        f[k] = c - (double)i0[k];
        flat[k] = raw < 0.0 || raw > (double)last || last == 0;
    }
    auto node = [&](int x, int y, int z) -> const float * {
        return t.coeffs + 3 * ((size_t)x + (size_t)t.dims[0] * ((size_t)y + (size_t)t.dims[1] * (size_t)z));
    };
    const float *n000 = node(i0[0], i0[1], i0[2]), *n100 = node(i1[0], i0[1], i0[2]), *n010 = node(i0[0], i1[1], i0[2]),
                *n110 = node(i1[0], i1[1], i0[2]), *n001 = node(i0[0], i0[1], i1[2]), *n101 = node(i1[0], i0[1], i1[2]),
                *n011 = node(i0[0], i1[1], i1[2]), *n111 = node(i1[0], i1[1], i1[2]);
    const double fx = f[0], fy = f[1], fz = f[2];
    const double rx = 1 - fx, ry = 1 - fy, rz = 1 - fz;
    for (int r = 0; r < 3; r++) {
        const double a = n000[r], b = n100[r], c = n010[r], d = n110[r], e = n001[r], g = n101[r], h = n011[r], m = n111[r];
        const double v = rz * (ry * (rx * a + fx * b) + fy * (rx * c + fx * d))
                       + fz * (ry * (rx * e + fx * g) + fy * (rx * h + fx * m));
        q[r] = p[r] + v;
        if (JAC) {
            const double gx = rz * (ry * (b - a) + fy * (d - c)) + fz * (ry * (g - e) + fy * (m - h));
            const double gy = rz * (rx * (c - a) + fx * (d - b)) + fz * (rx * (h - e) + fx * (m - g));
            const double gz = ry * (rx * (e - a) + fx * (g - b)) + fy * (rx * (h - c) + fx * (m - d));
            J[r][0] = (r == 0 ? 1.0 : 0.0) + (flat[0] ? 0.0 : gx / t.spacing[0]);
            J[r][1] = (r == 1 ? 1.0 : 0.0) + (flat[1] ? 0.0 : gy / t.spacing[1]);
            J[r][2] = (r == 2 ? 1.0 : 0.0) + (flat[2] ? 0.0 : gz / t.spacing[2]);
        }
    }
}

// a B-spline lattice, forward: q = p + d(p), J = I + dd/dp
template <bool JAC>
__device__ __forceinline__ void bspline_forward(const DevLink &t, const double p[3], double q[3], double J[3][3])
{
    double F[3][4], G[3][4];
    int i0[3];
    for (int k = 0; k < 3; k++) {
        // clamped before the int conversion (undefined beyond 2^31 cells, and for NaN): below -2 or from dims + 1 on no tap
        // touches the lattice either way, so d = 0 and q = p (NaN stays NaN) exactly as without the clamp
        const double u = fmin(fmax((p[k] - t.origin[k]) / t.spacing[k], -3.0), (double)t.dims[k] + 1.0);
        const double fl = floor(u);
        i0[k] = (int)fl - 1;
        basis(u - fl, F[k], G[k]);
    }
    double d[3] = { 0, 0, 0 }, dd[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
    for (int k = 0; k < 4; k++) {
        const int z = i0[2] + k;
        if (z < 0 || z >= t.dims[2]) continue;
        for (int j = 0; j < 4; j++) {
            const int y = i0[1] + j;
            if (y < 0 || y >= t.dims[1]) continue;
            for (int i = 0; i < 4; i++) {
                const int x = i0[0] + i;
                if (x < 0 || x >= t.dims[0]) continue;
                const float *c = t.coeffs + 3 * ((size_t)x + (size_t)t.dims[0] * ((size_t)y + (size_t)t.dims[1] * (size_t)z));
                const double w = F[0][i] * F[1][j] * F[2][k];
                const double c0 = c[0], c1 = c[1], c2 = c[2];
                d[0] += w * c0; d[1] += w * c1; d[2] += w * c2;
                if (JAC) {
                    const double wx = G[0][i] * F[1][j] * F[2][k], wy = F[0][i] * G[1][j] * F[2][k], wz = F[0][i] * F[1][j] * G[2][k];
                    dd[0][0] += wx * c0; dd[0][1] += wy * c0; dd[0][2] += wz * c0;
                    dd[1][0] += wx * c1; dd[1][1] += wy * c1; dd[1][2] += wz * c1;
                    dd[2][0] += wx * c2; dd[2][1] += wy * c2; dd[2][2] += wz * c2;
                }
            }
        }
    }
    for (int r = 0; r < 3; r++) {
        q[r] = p[r] + d[r];
        if (JAC) for (int c = 0; c < 3; c++) J[r][c] = (r == c ? 1.0 : 0.0) + dd[r][c] / t.spacing[c];
    }
}

// one link, forward: q = T(p), J = dT/dp
template <bool JAC>
__device__ __forceinline__ void link_forward(const DevLink &t, const double p[3], double q[3], double J[3][3])
{
    if (t.type == FROG_T_LINEAR) {
        for (int r = 0; r < 3; r++) {
            q[r] = t.m[4 * r] * p[0] + t.m[4 * r + 1] * p[1] + t.m[4 * r + 2] * p[2] + t.m[4 * r + 3];
            if (JAC) for (int c = 0; c < 3; c++) J[r][c] = t.m[4 * r + c];
        }
        return;
    }
    if (t.type == FROG_T_FIELD) field_forward<JAC>(t, p, q, J);
    else bspline_forward<JAC>(t, p, q, J);
}

// delta = J^-1 r  (Cramer; the lattices frog writes with -gd 1 have det J > 0)
__device__ __forceinline__ void solve3(const double J[3][3], const double r[3], double delta[3])
{
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                 c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double inv = 1.0 / det;
    delta[0] = (c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2]) * inv;
    delta[1] = (c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2]) * inv;
    delta[2] = (c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2]) * inv;
}

// Inverse of a B-spline link: the x with T(x) = p, by Newton's method with the step-halving safeguard
// vtkWarpTransform uses for its inverses (first guess x = p - d(p); a step that increases |T(x) - p|^2 is
// shortened by a factor from the parabola through the last two values, clamped to [0.1, 0.5]; stop when
// both the step and the residual are below the tolerance, VTK's default 1e-3, or after 500 iterations,
// then fall back to the best point seen).  q = x, J = (dT/dx)^-1 at x.
template <bool JAC>
__device__ void bspline_inverse(const DevLink &t, const double p[3], double q[3], double Jinv[3][3])
{
    const double tol2 = INVERSE_TOLERANCE * INVERSE_TOLERANCE;
    double x[3], fx[3], J[3][3], r[3], delta[3] = { 0, 0, 0 }, last_x[3], last_f = 0, fderiv = 0, frac = 1;
    bspline_forward<false>(t, p, fx, J);
    for (int k = 0; k < 3; k++) { x[k] = p[k] - (fx[k] - p[k]); last_x[k] = x[k]; }
    int it = 0;
    for (; it < INVERSE_ITERATIONS; it++) {
        bspline_forward<true>(t, x, fx, J);
        for (int k = 0; k < 3; k++) r[k] = fx[k] - p[k];
        const double fval = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        if (it == 0 || fval < last_f) {
            solve3(J, r, delta);
            const double err2 = delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2];
            if (err2 < tol2 && fval < tol2) break;
            for (int k = 0; k < 3; k++) last_x[k] = x[k];
            last_f = fval;
            // derivative of |T(x) - p|^2 along -delta at the last point: -2 r.(J delta) = -2 |r|^2
            fderiv = -2.0 * fval;
            for (int k = 0; k < 3; k++) x[k] -= delta[k];
            frac = 1.0;
            continue;
        }
        double a = -fderiv / (2.0 * (fval - last_f - fderiv));
        a = a < 0.1 ? 0.1 : (a > 0.5 ? 0.5 : a);
        frac *= a;
        for (int k = 0; k < 3; k++) x[k] = last_x[k] - frac * delta[k];
    }
    if (it >= INVERSE_ITERATIONS) for (int k = 0; k < 3; k++) x[k] = last_x[k];      // did not converge: best point seen
    for (int k = 0; k < 3; k++) q[k] = x[k];
    if (JAC) {
        bspline_forward<true>(t, x, fx, J);
        for (int c = 0; c < 3; c++) {
            const double e[3] = { c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0 };
            double col[3];
            solve3(J, e, col);
            for (int rr = 0; rr < 3; rr++) Jinv[rr][c] = col[rr];
        }
    }
}

template <bool JAC>
__device__ void chain_point(const DevLink *links, int n_links, double p[3], double A[3][3])
{
    if (JAC) { A[0][0] = A[1][1] = A[2][2] = 1; A[0][1] = A[0][2] = A[1][0] = A[1][2] = A[2][0] = A[2][1] = 0; }
    for (int l = 0; l < n_links; l++) {
        const DevLink &t = links[l];
        double q[3], J[3][3];
        if (t.type == FROG_T_BSPLINE_INVERSE) bspline_inverse<JAC>(t, p, q, J);
        else link_forward<JAC>(t, p, q, J);
        if (JAC) {
            double B[3][3];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) B[r][c] = J[r][0] * A[0][c] + J[r][1] * A[1][c] + J[r][2] * A[2][c];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) A[r][c] = B[r][c];
        }
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
}

// A regular grid of nodes, x fastest: what frog_chain_check and frog_chain_sample evaluate the chain on, and the output
// side of a reslice.
struct NodeGrid {
    double origin[3], spacing[3];
    uint32_t dims[3];
};

// node idx of the grid: p = origin + (i, j, k) * spacing
__device__ __forceinline__ void grid_node(const NodeGrid &g, size_t idx, double p[3])
{
    const uint32_t nx = g.dims[0], ny = g.dims[1];
    const uint32_t i = (uint32_t)(idx % nx), j = (uint32_t)((idx / nx) % ny), k = (uint32_t)(idx / ((size_t)nx * ny));
    p[0] = g.origin[0] + i * g.spacing[0]; p[1] = g.origin[1] + j * g.spacing[1]; p[2] = g.origin[2] + k * g.spacing[2];
}

// cofactor expansion along the first row
__device__ __forceinline__ double det3(const double A[3][3])
{
    return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
         + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// ---- vtkImageReslice as tools/VolumeTransform.cxx:119-136 configures it ------------------------------------
// One thread per output voxel: its position in the reference volume's frame goes through the chain (which
// maps output space to source space), the source is sampled there in its own scalar type, the arithmetic is
// f64, the result goes back to that type (integers: rounded half up and clamped, as vtkImageReslice does).
// Inside test with VTK's default
// half-voxel border: a sample up to half a voxel outside the first/last voxel centre still reads the
// edge value (indices clamped); further out it is `background`.
template <class S>
__device__ __forceinline__ S to_voxel(double v)
{
    if constexpr (std::is_integral<S>::value) {
        const double lo = (double)std::numeric_limits<S>::lowest(), hi = (double)std::numeric_limits<S>::max();
        double x = floor(v + 0.5);
        x = x < lo ? lo : (x > hi ? hi : x);
        return (S)x;
    } else {
        return (S)v;
    }
}

// Geometry of one reslice: the source's voxel grid (s*) and the output grid, as frog_volume gives them.
struct ResliceGrid {
    int sx, sy, sz;
    double so[3], ss[3];
    NodeGrid out;
    int linear;
    double background;
};

// The position of output voxel idx (x fastest) after the chain, in the space of whatever is sampled there.
__device__ __forceinline__ void reslice_position(const DevLink *links, int n_links, const NodeGrid &out, size_t idx, double p[3])
{
    double A[3][3];
    grid_node(out, idx, p);
    chain_point<false>(links, n_links, p, A);
}

// p in the voxel coordinates of a volume (dims sx, sy, sz at origin o, spacing s), and the inside test with the half-voxel
// border.  A NaN coordinate fails it.
__device__ __forceinline__ bool voxel_coordinates(const double p[3], const double o[3], const double s[3], int sx, int sy, int sz, double c[3])
{
    c[0] = (p[0] - o[0]) / s[0]; c[1] = (p[1] - o[1]) / s[1]; c[2] = (p[2] - o[2]) / s[2];
    const int dims[3] = { sx, sy, sz };
    bool inside = true;
    for (int a = 0; a < 3; a++) inside = inside && c[a] >= -0.5 && c[a] <= (double)dims[a] - 0.5;
    return inside;
}

// The voxel a reslice stores for a sample at voxel coordinates c of the source: the background where it is not inside.
template <class S>
__device__ __forceinline__ S reslice_sample(const S *__restrict__ src, const ResliceGrid &g, const double c[3], bool inside)
{
    const int sx = g.sx, sy = g.sy, sz = g.sz;
    double v = g.background;
    if (inside) {
        auto at = [&](int x, int y, int z) -> double {
            x = x < 0 ? 0 : (x >= sx ? sx - 1 : x);
            y = y < 0 ? 0 : (y >= sy ? sy - 1 : y);
            z = z < 0 ? 0 : (z >= sz ? sz - 1 : z);
            return (double)src[(size_t)x + (size_t)sx * ((size_t)y + (size_t)sy * (size_t)z)];
        };
        if (!g.linear) {
            v = at((int)floor(c[0] + 0.5), (int)floor(c[1] + 0.5), (int)floor(c[2] + 0.5));
        } else {
            const double f0 = floor(c[0]), f1 = floor(c[1]), f2 = floor(c[2]);
            const int x0 = (int)f0, y0 = (int)f1, z0 = (int)f2;
            const double fx = c[0] - f0, fy = c[1] - f1, fz = c[2] - f2;
            const double rx = 1 - fx, ry = 1 - fy, rz = 1 - fz;
            v = rz * (ry * (rx * at(x0, y0, z0) + fx * at(x0 + 1, y0, z0)) + fy * (rx * at(x0, y0 + 1, z0) + fx * at(x0 + 1, y0 + 1, z0)))
              + fz * (ry * (rx * at(x0, y0, z0 + 1) + fx * at(x0 + 1, y0, z0 + 1)) + fy * (rx * at(x0, y0 + 1, z0 + 1) + fx * at(x0 + 1, y0 + 1, z0 + 1)));
        }
    }
    return to_voxel<S>(v);
}

// Output voxel idx (x fastest) of a reslice: what reslice_kernel stores and reslice_accumulate_kernel adds.
template <class S>
__device__ __forceinline__ S reslice_voxel(const DevLink *links, int n_links, const S *__restrict__ src, const ResliceGrid &g, size_t idx)
{
    double p[3], c[3];
    reslice_position(links, n_links, g.out, idx, p);
    const bool inside = voxel_coordinates(p, g.so, g.ss, g.sx, g.sy, g.sz, c);
    return reslice_sample<S>(src, g, c, inside);
}

template <class S>
__global__ __launch_bounds__(256) void reslice_kernel(size_t base, const DevLink *links, int n_links, const S *__restrict__ src,
                                                      const ResliceGrid g, S *__restrict__ out)
{
    const size_t total = (size_t)g.out.dims[0] * g.out.dims[1] * g.out.dims[2];
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    out[idx] = reslice_voxel<S>(links, n_links, src, g, idx);
}

// ---- mean / stdev of a registered group (tools/AverageVolumes.cxx:47-59, :68-74) -----------------------------------------
// One thread owns one voxel of the two f32 accumulators: the images are added in call order, no atomics, so the sums are
// the reference's own sequence.  Each value goes to float first (vtkImageCast), then avg += v / n, sq += (v * v) / n with
// n = (float)n_images; -ffp-contract=off keeps the product and the quotient separately rounded (no FMA), and gfx950's
// f32 division and sqrt are the correctly rounded sequences under -fno-fast-math.
template <class S>
__device__ __forceinline__ void accumulate(float *__restrict__ avg, float *__restrict__ sq, size_t idx, S value, float n)
{
    const float v = (float)value;
    avg[idx] += v / n;
    sq[idx] += (v * v) / n;
}

// the source resliced onto the grid (reslice_voxel, the same code as reslice_kernel), then added; `out` (may be null)
// receives the resliced voxel in the source's type, what VolumeTransform would have written
template <class S>
__global__ __launch_bounds__(256) void reslice_accumulate_kernel(size_t base, const DevLink *links, int n_links, const S *__restrict__ src,
                                                                 const ResliceGrid g, float n, float *__restrict__ avg,
                                                                 float *__restrict__ sq, S *__restrict__ out)
{
    const size_t total = (size_t)g.out.dims[0] * g.out.dims[1] * g.out.dims[2];
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const S r = reslice_voxel<S>(links, n_links, src, g, idx);
    if (out) out[idx] = r;
    accumulate<S>(avg, sq, idx, r, n);
}

// a source already on the grid (AverageVolumes' own inputs)
template <class S>
__global__ __launch_bounds__(256) void identity_accumulate_kernel(size_t base, const S *__restrict__ src, size_t total, float n,
                                                                  float *__restrict__ avg, float *__restrict__ sq)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    accumulate<S>(avg, sq, idx, src[idx], n);
}

// stdev = sqrt(sq - avg * avg) in place of sq: NaN where the f32 difference rounds negative, as in the reference
__global__ __launch_bounds__(256) void average_finish_kernel(size_t base, const float *__restrict__ avg, float *__restrict__ sq, size_t total)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float a = avg[idx];
    const float a2 = a * a;
    sq[idx] = sqrtf(sq[idx] - a2);
}

// ---- mean / stdev / count over the images that cover a voxel (frog_cover; no counterpart in the reference) -----------------
// Three accumulators per voxel, owned by one thread as in accumulate: the running mean and sum of squared deviations
// (Welford) and the number of images that were valid there.  One f32 operation per statement (-ffp-contract=off), in the
// order include/frog_chain.h states.  The new mean is a rounded value between the old mean and x (rounding is monotone), so
// x - mean_new has d's sign or is zero, d * (x - mean_new) >= 0 and m2 never decreases: sqrtf(m2 / k) has no difference
// under the root and gives no NaN unless a difference overflows.
__device__ __forceinline__ void cover_update(float *__restrict__ mean, float *__restrict__ m2, uint16_t *__restrict__ count, size_t idx, float x)
{
    const uint32_t k = (uint32_t)count[idx] + 1u;
    const float m = mean[idx];
    const float d = x - m;
    const float q = d / (float)k;
    const float m_new = m + q;
    const float e = x - m_new;
    const float t = d * e;
    mean[idx] = m_new;
    m2[idx] = m2[idx] + t;
    count[idx] = (uint16_t)k;
}

// The geometry of a mask (u8, non-zero = valid), which need not be the source's.
struct MaskGrid {
    int sx, sy, sz;
    double so[3], ss[3];
};

// Whether the mask counts position p (after the chain): inside the mask's own geometry and its nearest voxel non-zero.
__device__ __forceinline__ bool mask_covers(const double p[3], const uint8_t *__restrict__ mask, const MaskGrid &mg)
{
    double c[3];
    if (!voxel_coordinates(p, mg.so, mg.ss, mg.sx, mg.sy, mg.sz, c)) return false;
    int x = (int)floor(c[0] + 0.5), y = (int)floor(c[1] + 0.5), z = (int)floor(c[2] + 0.5);
    x = x < 0 ? 0 : (x >= mg.sx ? mg.sx - 1 : x);
    y = y < 0 ? 0 : (y >= mg.sy ? mg.sy - 1 : y);
    z = z < 0 ? 0 : (z >= mg.sz ? mg.sz - 1 : z);
    return mask[(size_t)x + (size_t)mg.sx * ((size_t)y + (size_t)mg.sy * (size_t)z)] != 0;
}

// The chain is evaluated once: the position it gives is turned into the source's voxel coordinates (reslice_sample, the code
// of reslice_kernel, gives the value and `out`) and, where the source covers it, into the mask's, whose nearest voxel
// (floor(c + 0.5), as a nearest-neighbour reslice reads it) decides.
template <class S>
__global__ __launch_bounds__(256) void cover_reslice_kernel(size_t base, const DevLink *links, int n_links, const S *__restrict__ src,
                                                            const ResliceGrid g, const uint8_t *__restrict__ mask, const MaskGrid mg,
                                                            float *__restrict__ mean, float *__restrict__ m2,
                                                            uint16_t *__restrict__ count, S *__restrict__ out)
{
    const size_t total = (size_t)g.out.dims[0] * g.out.dims[1] * g.out.dims[2];
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    double p[3], c[3];
    reslice_position(links, n_links, g.out, idx, p);
    bool valid = voxel_coordinates(p, g.so, g.ss, g.sx, g.sy, g.sz, c);
    const S r = reslice_sample<S>(src, g, c, valid);
    if (out) out[idx] = r;
    if (valid && mask) valid = mask_covers(p, mask, mg);
    if (valid) cover_update(mean, m2, count, idx, (float)r);
}

// a source (and a mask) already on the grid: every voxel is inside
template <class S>
__global__ __launch_bounds__(256) void cover_identity_kernel(size_t base, const S *__restrict__ src, const uint8_t *__restrict__ mask, size_t total,
                                                             float *__restrict__ mean, float *__restrict__ m2, uint16_t *__restrict__ count)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    if (!mask || mask[idx] != 0) cover_update(mean, m2, count, idx, (float)src[idx]);
}

// where count >= min_count the mean as held and sqrt(m2 / count), elsewhere `fill` and 0; any output may be null
__global__ __launch_bounds__(256) void cover_finish_kernel(size_t base, const float *__restrict__ mean, const float *__restrict__ m2,
                                                           const uint16_t *__restrict__ count, size_t total, uint32_t min_count, float fill,
                                                           float *__restrict__ out_mean, float *__restrict__ out_stdev)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t k = count[idx];
    const bool enough = k >= min_count;
    if (out_mean) out_mean[idx] = enough ? mean[idx] : fill;
    if (out_stdev) {
        float s = 0.0f;
        if (enough) {
            const float variance = m2[idx] / (float)k;
            s = sqrtf(variance);
        }
        out_stdev[idx] = s;
    }
}

// ---- one image against the accumulator's mean (frog_cover_score) ------------------------------------------------------------
// A reduction over the volume instead of a volume: per voxel the value x the add would have used and the reference y formed
// from the held mean and count, six f64 sums and two counts per TILE of SCORE_TILE consecutive voxels, and a joint histogram.
// No floating-point atomic anywhere: the order of every f64 addition is the one include/frog_chain.h states (thread, then
// the wave's shuffle tree, then the four waves, then -- on the host -- the tiles), and a block is a tile whatever the launch
// chunk, so the sums do not depend on scheduling or on FROG_CHAIN_LAUNCH_MAX.  The histogram is integer: one u32 image in LDS
// per block, LDS atomics, one 64-bit global atomic per non-zero bin and block.
constexpr int SCORE_ITEMS = 8;                              // voxels per thread
constexpr size_t SCORE_TILE = SCORE_ITEMS * 256;            // voxels per block

struct ScorePartial {           // one tile: seven 8-byte words
    double s[6];                // sx sy sxx syy sxy sad
    uint32_t n, n_nonfinite;
};

struct ScoreParams {
    uint32_t need;              // the smallest count that takes part: max(2 or 1, min_count)
    int leave_one_out;
    uint32_t bins;              // 0: no histogram
    float lo, scale;            // scale = (float)bins / (hi - lo)
};

// min(bins - 1, max(0, floorf((t - lo) * scale))), clamped before the conversion to int (t may be +-inf after a cast)
__device__ __forceinline__ uint32_t score_bin(const ScoreParams &sp, float t)
{
    const float d = t - sp.lo;
    const float f = floorf(d * sp.scale);
    return !(f >= 0.0f) ? 0u : (f >= (float)sp.bins ? sp.bins - 1u : (uint32_t)f);
}

// one voxel whose image is valid there: x against the accumulator's (m, k)
__device__ __forceinline__ void score_voxel(const ScoreParams &sp, float x, float m, uint32_t k, ScorePartial &acc, uint32_t *hist)
{
    if (k < sp.need) return;
    const double xd = (double)x;
    double y = (double)m;
    if (sp.leave_one_out) {
        const double mk = y * (double)k;
        const double others = mk - xd;
        y = others / (double)(k - 1u);
    }
    if (!(isfinite(xd) && isfinite(y))) { acc.n_nonfinite++; return; }
    const double xx = xd * xd, yy = y * y, xy = xd * y, diff = xd - y;
    acc.n++;
    acc.s[0] += xd; acc.s[1] += y; acc.s[2] += xx; acc.s[3] += yy; acc.s[4] += xy; acc.s[5] += fabs(diff);
    if (sp.bins) atomicAdd(&hist[score_bin(sp, x) * sp.bins + score_bin(sp, (float)y)], 1u);
}

// The block's end: lane 0 of each wave gets the wave's sums by __shfl_down 32, 16, 8, 4, 2, 1, thread 0 adds the four waves
// in ascending order into partials[tile], and the LDS histogram's non-zero bins go to the device histogram.
__device__ __forceinline__ void score_block_end(ScorePartial &acc, size_t tile, uint32_t cells, const uint32_t *hist,
                                                ScorePartial *__restrict__ partials, unsigned long long *__restrict__ histogram)
{
    __shared__ ScorePartial waves[4];
    for (int h = 32; h > 0; h >>= 1) {
        for (int q = 0; q < 6; q++) acc.s[q] += __shfl_down(acc.s[q], h);
        acc.n += __shfl_down(acc.n, h);
        acc.n_nonfinite += __shfl_down(acc.n_nonfinite, h);
    }
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();                                        // also: every LDS histogram update of the block is done
    if (threadIdx.x == 0) {
        ScorePartial t = waves[0];
        for (int w = 1; w < 4; w++) {
            for (int q = 0; q < 6; q++) t.s[q] += waves[w].s[q];
            t.n += waves[w].n;
            t.n_nonfinite += waves[w].n_nonfinite;
        }
        partials[tile] = t;
    }
    for (uint32_t b = threadIdx.x; b < cells; b += 256) {
        const uint32_t c = hist[b];
        if (c) atomicAdd(&histogram[b], (unsigned long long)c);
    }
}

// validity and value exactly as cover_reslice_kernel forms them; thread t of tile T takes voxels T * SCORE_TILE + j * 256 + t
template <class S>
__global__ __launch_bounds__(256) void cover_score_kernel(size_t base, const DevLink *links, int n_links, const S *__restrict__ src,
                                                          const ResliceGrid g, const uint8_t *__restrict__ mask, const MaskGrid mg,
                                                          const float *__restrict__ mean, const uint16_t *__restrict__ count,
                                                          const ScoreParams sp, ScorePartial *__restrict__ partials,
                                                          unsigned long long *__restrict__ histogram)
{
    extern __shared__ uint32_t score_hist[];
    const size_t total = (size_t)g.out.dims[0] * g.out.dims[1] * g.out.dims[2];
    const size_t tile = base / 256 + blockIdx.x;
    const uint32_t cells = sp.bins * sp.bins;
    for (uint32_t b = threadIdx.x; b < cells; b += 256) score_hist[b] = 0;
    __syncthreads();
    ScorePartial acc{};
#pragma unroll 1
    for (int j = 0; j < SCORE_ITEMS; j++) {
        const size_t idx = tile * SCORE_TILE + (size_t)j * 256 + threadIdx.x;
        if (idx >= total) break;
        double p[3], c[3];
        reslice_position(links, n_links, g.out, idx, p);
        bool valid = voxel_coordinates(p, g.so, g.ss, g.sx, g.sy, g.sz, c);
        const S r = reslice_sample<S>(src, g, c, valid);
        if (valid && mask) valid = mask_covers(p, mask, mg);
        if (valid) score_voxel(sp, (float)r, mean[idx], count[idx], acc, score_hist);
    }
    score_block_end(acc, tile, cells, score_hist, partials, histogram);
}

// a source (and a mask) already on the grid: every voxel is inside
template <class S>
__global__ __launch_bounds__(256) void cover_score_identity_kernel(size_t base, const S *__restrict__ src, const uint8_t *__restrict__ mask,
                                                                   size_t total, const float *__restrict__ mean,
                                                                   const uint16_t *__restrict__ count, const ScoreParams sp,
                                                                   ScorePartial *__restrict__ partials, unsigned long long *__restrict__ histogram)
{
    extern __shared__ uint32_t score_hist[];
    const size_t tile = base / 256 + blockIdx.x;
    const uint32_t cells = sp.bins * sp.bins;
    for (uint32_t b = threadIdx.x; b < cells; b += 256) score_hist[b] = 0;
    __syncthreads();
    ScorePartial acc{};
#pragma unroll
    for (int j = 0; j < SCORE_ITEMS; j++) {
        const size_t idx = tile * SCORE_TILE + (size_t)j * 256 + threadIdx.x;
        if (idx < total && (!mask || mask[idx] != 0)) score_voxel(sp, (float)src[idx], mean[idx], count[idx], acc, score_hist);
    }
    score_block_end(acc, tile, cells, score_hist, partials, histogram);
}

__global__ __launch_bounds__(256) void chain_apply_kernel(size_t base, const DevLink *links, int n_links, const double *in, double *out, size_t n)
{
    const size_t i = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[3] = { in[3 * i], in[3 * i + 1], in[3 * i + 2] }, A[3][3];
    chain_point<false>(links, n_links, p, A);
    out[3 * i] = p[0]; out[3 * i + 1] = p[1]; out[3 * i + 2] = p[2];
}

// one thread per grid node; block-level reduction of (negative count, minimum determinant) into the block's slot, numbered
// from the first block of the whole grid (base is a multiple of the block size: chunked_launch)
__global__ __launch_bounds__(256) void chain_check_kernel(size_t base, const DevLink *links, int n_links, const NodeGrid g,
                                                          unsigned long long *n_negative, double *block_min)
{
    __shared__ double mins[256];
    __shared__ unsigned int negs[256];
    const size_t total = (size_t)g.dims[0] * g.dims[1] * g.dims[2];
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double det = INFINITY;
    unsigned int neg = 0;
    if (idx < total) {
        double p[3], A[3][3];
        grid_node(g, idx, p);
        chain_point<true>(links, n_links, p, A);
        det = det3(A);
        neg = det < 0 ? 1u : 0u;
    }
    mins[threadIdx.x] = det; negs[threadIdx.x] = neg;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { mins[threadIdx.x] = fmin(mins[threadIdx.x], mins[threadIdx.x + h]); negs[threadIdx.x] += negs[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_min[base / 256 + blockIdx.x] = mins[0];
        if (negs[0]) atomicAdd(n_negative, (unsigned long long)negs[0]);
    }
}

// one thread per grid node of a slab [first, first + count) of the whole grid (first and base are multiples of the block size):
// the node and the determinant as chain_check_kernel computes them, the displacement as chain_apply_kernel's output minus the
// node, each stored with one cast.  DET selects chain_point<true>; without it no Jacobian is formed.
template <bool DISP, bool DET, class T>
__global__ __launch_bounds__(256) void chain_sample_kernel(size_t first, size_t base, size_t count, const DevLink *links, int n_links,
                                                           const NodeGrid g, T *__restrict__ displacement, T *__restrict__ determinant)
{
    const size_t local = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= count) return;
    const size_t idx = first + local;
    double p[3], A[3][3];
    grid_node(g, idx, p);
    const double node[3] = { p[0], p[1], p[2] };
    chain_point<DET>(links, n_links, p, A);
    if (DISP) {
        displacement[3 * local] = (T)(p[0] - node[0]);
        displacement[3 * local + 1] = (T)(p[1] - node[1]);
        displacement[3 * local + 2] = (T)(p[2] - node[2]);
    }
    if (DET) {
        determinant[local] = (T)det3(A);
    }
}

// ---- majority-vote fusion of a group's label maps (frog_labels; no counterpart in the reference) --------------------------
// Label values are sparse and unknown in advance (RadLex ids: 58, 1247, 40358, ...), so the distinct values are found on the
// device: an open-addressing map (linear probing, load <= 1/2) from the value to a dense plane index, kept across adds.  The
// dense indices depend on which thread inserts first; nothing that leaves the library depends on them (the table is sorted
// by value, ties go to the smaller value).  Per label one plane of 16-bit vote counts, x fastest like the grid.
constexpr long long LABEL_EMPTY = std::numeric_limits<long long>::min();     // no integer voxel type holds it
constexpr uint32_t LABEL_NONE = 0xFFFFFFFFu;
constexpr int LABEL_TABLE_ITEMS = 32;           // voxels per thread of labels_table_kernel
constexpr size_t LABEL_SUM_STRIDE = 32;        // u64 words between the sums of two labels

struct LabelMap {
    long long *keys;            // slot -> value, LABEL_EMPTY where free
    uint32_t *index;            // slot -> dense index
    long long *values;          // dense index -> value
    uint32_t *state;            // [0] dense indices handed out, [1] set when a value found no index or no slot
    uint32_t mask;              // slots - 1 (a power of two)
    int shift;                  // 64 - log2(slots)
    uint32_t max_labels;
};

// Fibonacci hashing: the high bits of the product, so that runs of k * 8192 or k * 65536 do not share a slot
__host__ __device__ __forceinline__ uint32_t label_slot(long long v, int shift)
{
    return (uint32_t)(((unsigned long long)v * 0x9E3779B97F4A7C15ull) >> shift);
}

// Makes `v` a key of the map.  Neighbouring voxels nearly always carry the same, already known label: a plain (L1) read of
// the slot settles those.  A slot that reads otherwise is read again at the L2 (a CU's L1 may still hold the line from
// before another CU's insert), and only a slot that is free there gets the compare-and-swap; the thread that wins it draws
// the dense index.  Once the state's flag is up the call has failed as a whole and the threads stop probing.
__device__ __forceinline__ void label_insert(const LabelMap &m, long long v)
{
    uint32_t slot = label_slot(v, m.shift);
    for (uint32_t probe = 0; probe <= m.mask; probe++, slot = (slot + 1) & m.mask) {
        if (m.keys[slot] == v) return;
        long long k = __hip_atomic_load(&m.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == LABEL_EMPTY)
            k = (long long)atomicCAS((unsigned long long *)&m.keys[slot], (unsigned long long)LABEL_EMPTY, (unsigned long long)v);
        else if (k != v && __hip_atomic_load(&m.state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (k == LABEL_EMPTY) {                         // this thread's insert
            const uint32_t idx = atomicAdd(&m.state[0], 1u);
            if (idx < m.max_labels) { m.index[slot] = idx; m.values[idx] = v; }
            else atomicExch(&m.state[1], 1u);
            return;
        }
        if (k == v) return;
    }
    atomicExch(&m.state[1], 1u);                        // every slot taken by other values
}

// the dense index of a key (between kernels the map is at rest: plain reads); LABEL_NONE if `v` is no key
__device__ __forceinline__ uint32_t label_find(const LabelMap &m, long long v)
{
    uint32_t slot = label_slot(v, m.shift);
    for (uint32_t probe = 0; probe <= m.mask; probe++, slot = (slot + 1) & m.mask) {
        const long long k = m.keys[slot];
        if (k == v) return m.index[slot];
        if (k == LABEL_EMPTY) break;
    }
    return LABEL_NONE;
}

// phase 1 of an add: the voxel's label (through the chain: reslice_voxel, the code of reslice_kernel, into `stage`; else the
// source's own voxel) becomes a key of the map
template <class S, bool CHAIN>
__global__ __launch_bounds__(256) void labels_collect_kernel(size_t base, const DevLink *links, int n_links, const S *__restrict__ src,
                                                             const ResliceGrid g, size_t total, S *__restrict__ stage, const LabelMap m)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    S label;
    if (CHAIN) {
        label = reslice_voxel<S>(links, n_links, src, g, idx);
        stage[idx] = label;
    } else {
        label = src[idx];
    }
    label_insert(m, (long long)label);
}

// phase 2: the image's vote.  The thread owns the voxel in every plane, as in accumulate: no atomic.
template <class S>
__global__ __launch_bounds__(256) void labels_vote_kernel(size_t base, const S *__restrict__ labels, size_t total, const LabelMap m,
                                                          uint16_t *const *__restrict__ planes, uint32_t n_planes)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t l = label_find(m, (long long)labels[idx]);
    if (l < n_planes) planes[l][idx] += 1;
}

// Per label sum of c and of c (c - 1) / 2 over the voxels, c the label's count: a block takes LABEL_TABLE_ITEMS * 256
// voxels of one plane (the work-items of a label are padded to whole blocks), two voxels per 4-byte load, reduces across the
// wave and through LDS and adds once per sum.  The sums of a label have a 256-byte row of their own (LABEL_SUM_STRIDE), so
// that the blocks' atomics spread over the memory channels.  Integer sums: the order of the blocks does not matter.
__global__ __launch_bounds__(256) void labels_table_kernel(size_t base, const uint16_t *const *__restrict__ planes, uint32_t n_planes,
                                                           size_t total, size_t blocks_per_plane, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long s_c[4], s_p[4];
    const size_t block = base / 256 + blockIdx.x;
    const size_t plane = block / blocks_per_plane, tile = block % blocks_per_plane;
    unsigned long long sc = 0, sp = 0;
    if (plane < n_planes) {
        const uint16_t *__restrict__ p = planes[plane];                 // hipMalloc's alignment: an even voxel is 4-byte aligned
        const size_t first = tile * LABEL_TABLE_ITEMS * 256 + 2 * threadIdx.x;
        uint32_t two[LABEL_TABLE_ITEMS / 2];
        if (first - 2 * threadIdx.x + LABEL_TABLE_ITEMS * 256 <= total) {           // a whole tile: every load issued before the first use
#pragma unroll
            for (int j = 0; j < LABEL_TABLE_ITEMS / 2; j++) __builtin_memcpy(&two[j], __builtin_assume_aligned(p + first + j * 512, 4), 4);
        } else {
            for (int j = 0; j < LABEL_TABLE_ITEMS / 2; j++) {
                const size_t v = first + j * 512;
                two[j] = 0;
                if (v + 1 < total) __builtin_memcpy(&two[j], __builtin_assume_aligned(p + v, 4), 4);
                else if (v < total) two[j] = p[v];
            }
        }
#pragma unroll
        for (int j = 0; j < LABEL_TABLE_ITEMS / 2; j++) {
            const unsigned long long c0 = two[j] & 0xFFFFu, c1 = two[j] >> 16;
            sc += c0 + c1;
            sp += (c0 * c0 - c0 + c1 * c1 - c1) / 2;                    // c (c - 1) is even: the sum halves exactly
        }
    }
    for (int h = 32; h > 0; h >>= 1) { sc += __shfl_down(sc, h); sp += __shfl_down(sp, h); }
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = sc; s_p[threadIdx.x >> 6] = sp; }
    __syncthreads();
    if (threadIdx.x == 0 && plane < n_planes) {
        sc = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        sp = s_p[0] + s_p[1] + s_p[2] + s_p[3];
        if (sc) atomicAdd(&sums[LABEL_SUM_STRIDE * plane], sc);
        if (sp) atomicAdd(&sums[LABEL_SUM_STRIDE * plane + 1], sp);
    }
}

// The winner of a voxel: `planes` and `values` in ascending order of the values, a later label must have strictly more
// votes, so a tie stays with the smallest value.  The loads of one plane are consecutive across the wave.
// agreement = (float)c / (float)n: one correctly rounded f32 division (see accumulate).
template <class T>
__global__ __launch_bounds__(256) void labels_fused_kernel(size_t base, const uint16_t *const *__restrict__ planes,
                                                           const long long *__restrict__ values, uint32_t n_labels, size_t total,
                                                           float n, T *__restrict__ label, float *__restrict__ agreement)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    uint32_t best = planes[0][idx], winner = 0;
    for (uint32_t l = 1; l < n_labels; l++) {
        const uint32_t c = planes[l][idx];
        if (c > best) { best = c; winner = l; }
    }
    if (label) label[idx] = (T)values[winner];
    if (agreement) agreement[idx] = (float)best / n;
}

__global__ __launch_bounds__(256) void labels_probability_kernel(size_t base, const uint16_t *__restrict__ plane, size_t total, float n,
                                                                 float *__restrict__ p)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    p[idx] = (float)plane[idx] / n;
}

// ---- locally weighted label fusion (frog_wlabels; no counterpart in the reference) -------------------------------------------
// An add has two phases.  Phase 1 evaluates the chain once per voxel and leaves the atlas on the grid: its image as an f32
// plane in which a voxel that is not valid (outside the source, or not finite) is a NaN -- a non-finite value is no member
// anyway, so the plane needs no mask beside it -- and its label map in the labels' own type, every label a key of the
// LabelMap.  Phase 2 (wlabels_vote_kernel) forms the patch sums from that plane and the target's and adds the weight to the
// label's plane.  The target's plane is made once by the kernel of phase 1 without the labels.

// a staged value: x = (float)r where the voxel is valid and x is finite, else NaN
template <class S>
__device__ __forceinline__ float wlabels_stage(S r, bool valid)
{
    const float x = (float)r;
    return valid && isfinite(x) ? x : __builtin_nanf("");
}

// voxel idx of a volume of one of the six integer types, picked at run time: one read per voxel, where 48 instantiations of a
// kernel that inlines the whole chain (image type x label type) would only lengthen the build
__device__ __forceinline__ long long label_load(const void *__restrict__ v, int dtype, size_t idx)
{
    switch (dtype) {
    case FROG_V_U8: return ((const uint8_t *)v)[idx];
    case FROG_V_I8: return ((const int8_t *)v)[idx];
    case FROG_V_U16: return ((const uint16_t *)v)[idx];
    case FROG_V_I16: return ((const int16_t *)v)[idx];
    case FROG_V_U32: return ((const uint32_t *)v)[idx];
    default: return ((const int32_t *)v)[idx];
    }
}

__device__ __forceinline__ void label_store(void *__restrict__ v, int dtype, size_t idx, long long label)
{
    switch (dtype) {
    case FROG_V_U8: ((uint8_t *)v)[idx] = (uint8_t)label; break;
    case FROG_V_I8: ((int8_t *)v)[idx] = (int8_t)label; break;
    case FROG_V_U16: ((uint16_t *)v)[idx] = (uint16_t)label; break;
    case FROG_V_I16: ((int16_t *)v)[idx] = (int16_t)label; break;
    case FROG_V_U32: ((uint32_t *)v)[idx] = (uint32_t)label; break;
    default: ((int32_t *)v)[idx] = (int32_t)label; break;
    }
}

// The voxel a nearest-neighbour reslice of the label map stores for position p (after the chain): reslice_sample's nearest
// branch with the type picked at run time.  An integer voxel passes to_voxel unchanged, so inside the map it is the voxel
// itself; outside it is the background rounded half up and clamped to the type.
__device__ __forceinline__ long long label_nearest(const void *__restrict__ src, int dtype, const ResliceGrid &g, const double p[3])
{
    double c[3];
    if (voxel_coordinates(p, g.so, g.ss, g.sx, g.sy, g.sz, c)) {
        int x = (int)floor(c[0] + 0.5), y = (int)floor(c[1] + 0.5), z = (int)floor(c[2] + 0.5);
        x = x < 0 ? 0 : (x >= g.sx ? g.sx - 1 : x);
        y = y < 0 ? 0 : (y >= g.sy ? g.sy - 1 : y);
        z = z < 0 ? 0 : (z >= g.sz ? g.sz - 1 : z);
        return label_load(src, dtype, (size_t)x + (size_t)g.sx * ((size_t)y + (size_t)g.sy * (size_t)z));
    }
    switch (dtype) {
    case FROG_V_U8: return to_voxel<uint8_t>(g.background);
    case FROG_V_I8: return to_voxel<int8_t>(g.background);
    case FROG_V_U16: return to_voxel<uint16_t>(g.background);
    case FROG_V_I16: return to_voxel<int16_t>(g.background);
    case FROG_V_U32: return to_voxel<uint32_t>(g.background);
    default: return to_voxel<int32_t>(g.background);
    }
}

// Phase 1.  LABELS false: the target.  The image goes through reslice_sample (the code of reslice_kernel) into `plane` (and,
// in its own type, into `out`, which may be null); with LABELS the label at the same position goes into `lout` in the
// labels' type and into the map.  Without a chain both volumes are on the grid: every voxel is inside, and phase 2 reads the
// labels where they are.
template <class S, bool CHAIN, bool LABELS>
__global__ __launch_bounds__(256) void wlabels_collect_kernel(size_t base, const DevLink *links, int n_links, const S *__restrict__ src,
                                                              const ResliceGrid g, const void *__restrict__ lsrc, int ltype, const ResliceGrid lg,
                                                              size_t total, float *__restrict__ plane, S *__restrict__ out,
                                                              void *__restrict__ lout, const LabelMap m)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    if (CHAIN) {
        double p[3], c[3];
        reslice_position(links, n_links, g.out, idx, p);
        const bool valid = voxel_coordinates(p, g.so, g.ss, g.sx, g.sy, g.sz, c);
        const S r = reslice_sample<S>(src, g, c, valid);
        if (out) out[idx] = r;
        plane[idx] = wlabels_stage<S>(r, valid);
        if (LABELS) {
            const long long label = label_nearest(lsrc, ltype, lg, p);
            label_store(lout, ltype, idx, label);
            label_insert(m, label);
        }
    } else {
        plane[idx] = wlabels_stage<S>(src[idx], true);
        if (LABELS) label_insert(m, label_load(lsrc, ltype, idx));
    }
}

// Phase 2, the vote.  A block owns a tile of 32 x 8 x 4 voxels (x fastest), thread (lx, ly) the column of its four z.  The
// tile and a halo of R voxels go to LDS as one (T, A) pair per voxel -- T a NaN where the voxel is no member of the patch
// (outside the grid, or the target or the atlas not valid there), A then 0 -- so a tap is one 8-byte LDS read, and the 32
// lanes of a lane group read 32 consecutive pairs: no bank conflict whatever the row length.  With the halo of R = 4 the
// tile holds 40 x 16 x 12 pairs = 61 440 bytes, within 64 KB; a tile 64 wide would need 72 x 12 x 12 pairs, 82 944 bytes.
// The six sums run over z, then y, then x ascending as the header states; a non-member adds +0.0 (and 0 to the count), which
// leaves every sum's bits as skipping it does: they start at +0.0 and never become -0.0.  One f64 operation per statement
// (-ffp-contract=off); the thread owns its voxel in every plane: no atomic.
constexpr int WL_TX = 32, WL_TY = 8, WL_TZ = 4;

struct WlabelsTiles {
    uint32_t nx, ny, nz;            // the grid
    uint32_t tx, ty;                // tiles along x and y
    size_t tiles;
};

template <int R>
__global__ __launch_bounds__(256) void wlabels_vote_kernel(size_t base, const float *__restrict__ target, const float *__restrict__ atlas,
                                                           const void *__restrict__ labels, int ltype, const WlabelsTiles w,
                                                           uint32_t power, float floor_c, const LabelMap m,
                                                           float *const *__restrict__ planes, uint32_t n_planes)
{
    constexpr int HX = WL_TX + 2 * R, HY = WL_TY + 2 * R, HZ = WL_TZ + 2 * R;
    __shared__ float2 s_ta[HX * HY * HZ];
    const size_t tile = base / 256 + blockIdx.x;            // one block per tile: the same for every thread of the block
    if (tile >= w.tiles) return;
    const int x0 = (int)(tile % w.tx) * WL_TX, y0 = (int)((tile / w.tx) % w.ty) * WL_TY, z0 = (int)(tile / ((size_t)w.tx * w.ty)) * WL_TZ;
    for (int i = threadIdx.x; i < HX * HY * HZ; i += 256) {
        const int x = x0 - R + i % HX, y = y0 - R + (i / HX) % HY, z = z0 - R + i / (HX * HY);
        float2 ta = make_float2(__builtin_nanf(""), 0.0f);
        if (x >= 0 && y >= 0 && z >= 0 && x < (int)w.nx && y < (int)w.ny && z < (int)w.nz) {
            const size_t idx = (size_t)x + (size_t)w.nx * ((size_t)y + (size_t)w.ny * (size_t)z);
            const float t = target[idx], a = atlas[idx];
            if (t == t && a == a) ta = make_float2(t, a);
        }
        s_ta[i] = ta;
    }
    __syncthreads();
    const int lx = threadIdx.x % WL_TX, ly = threadIdx.x / WL_TX;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= (int)w.nx || y >= (int)w.ny) return;
    for (int lz = 0; lz < WL_TZ && z0 + lz < (int)w.nz; lz++) {
        const float2 centre = s_ta[((lz + R) * HY + ly + R) * HX + lx + R];
        if (!(centre.x == centre.x)) continue;              // no member: no vote from this atlas
        uint32_t count = 0;
        double st = 0.0, sa = 0.0, stt = 0.0, saa = 0.0, sta = 0.0;
        for (int dz = 0; dz <= 2 * R; dz++) {
            for (int dy = 0; dy <= 2 * R; dy++) {
                const float2 *row = &s_ta[((lz + dz) * HY + ly + dy) * HX + lx];
#pragma unroll
                for (int dx = 0; dx <= 2 * R; dx++) {
                    const float2 ta = row[dx];
                    const bool member = ta.x == ta.x;
                    const double T = member ? (double)ta.x : 0.0, A = (double)ta.y;
                    const double tt = T * T, aa = A * A, tA = T * A;
                    count += member ? 1u : 0u;
                    st = st + T; sa = sa + A; stt = stt + tt; saa = saa + aa; sta = sta + tA;
                }
            }
        }
        const double n = (double)count;
        const double cov = n * sta - st * sa, vt = n * stt - st * st, va = n * saa - sa * sa;
        float c = 0.0f;
        if (count >= 2 && vt > 0.0 && va > 0.0 && cov > 0.0) {
            const double num = cov * cov, den = vt * va;
            const float q = (float)(num / den);
            c = sqrtf(q);
            if (isfinite(c)) c = fminf(c, 1.0f);
        }
        c = fmaxf(c, floor_c);
        float weight = c;
        for (uint32_t k = 1; k < power; k++) weight = weight * c;
        const size_t idx = (size_t)x + (size_t)w.nx * ((size_t)y + (size_t)w.ny * (size_t)(z0 + lz));
        const uint32_t l = label_find(m, label_load(labels, ltype, idx));
        if (l < n_planes) planes[l][idx] = planes[l][idx] + weight;
    }
}

// The winner of a voxel and its share: `planes` and `values` in ascending order of the values.  total is the planes' f32 sum
// in that order from +0.0; a later label must have a strictly larger score, and the first must be > 0, so a tie stays with
// the smallest value.  No weight at all: the fill label and 0.
template <class T>
__global__ __launch_bounds__(256) void wlabels_fused_kernel(size_t base, const float *const *__restrict__ planes,
                                                            const long long *__restrict__ values, uint32_t n_labels, size_t total,
                                                            T fill, T *__restrict__ label, float *__restrict__ confidence)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    float sum = 0.0f, best = 0.0f;
    uint32_t winner = 0;
    for (uint32_t l = 0; l < n_labels; l++) {
        const float s = planes[l][idx];
        sum = sum + s;
        if (s > best) { best = s; winner = l; }
    }
    const bool some = sum != 0.0f;
    if (label) label[idx] = some ? (T)values[winner] : fill;
    if (confidence) confidence[idx] = some ? best / sum : 0.0f;
}

// score / total of label `which` of the sorted planes; 0 where no weight arrived
__global__ __launch_bounds__(256) void wlabels_probability_kernel(size_t base, const float *const *__restrict__ planes, uint32_t n_labels,
                                                                  uint32_t which, size_t total, float *__restrict__ p)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    float sum = 0.0f, score = 0.0f;
    for (uint32_t l = 0; l < n_labels; l++) {
        const float s = planes[l][idx];
        sum = sum + s;
        if (l == which) score = s;
    }
    p[idx] = sum != 0.0f ? score / sum : 0.0f;
}

#include "k_rank.hip.h"
#include "k_staple.hip.h"
#include "k_edt.hip.h"
#include "k_joint.hip.h"
#include "k_glm.hip.h"
#include "k_ccl.hip.h"
#include "k_tfce.hip.h"
#include "k_smooth.hip.h"
#include "k_modes.hip.h"
#include "k_iso.hip.h"
#include "k_mesh.hip.h"

} // namespace

struct frog_chain {
    int device = 0;
    std::vector<DevLink> h_links;
    std::deque<frog::DevBuf<float>> d_coeffs;       // one per lattice or field link; a deque never copies its elements
    frog::DevBuf<DevLink> d_links;
};

// What every group accumulator holds: its device and grid, and the staging of the volume an add was given.
struct frog_group {
    int device = 0;
    frog_volume grid;
    size_t total = 0;
    frog::DevBuf<unsigned char> d_src, d_out;       // staging of the current source / resliced volume, grown on demand
};

// mean and stdev of a group on one grid
struct frog_average : frog_group {
    uint32_t n_images = 0, added = 0;
    bool finished = false;
    frog::DevBuf<float> d_avg, d_sq;
};

// an accumulator whose adds take a mask (frog_cover, frog_rank, frog_glm)
struct frog_masked : frog_group {
    frog::DevBuf<unsigned char> d_mask;             // staging of the current u8 mask, grown on demand
    std::vector<unsigned char> h_mask;              // the mask as value != 0, before its upload
};

// running mean, squared deviations and count of the images that cover each voxel of one grid
struct frog_cover : frog_masked {
    uint32_t added = 0;
    frog::DevBuf<float> d_mean, d_m2;
    frog::DevBuf<uint16_t> d_count;
};

// an accumulator that stores one plane per added image over a window of z-planes of one grid (frog_rank, frog_glm)
struct frog_windowed : frog_masked {
    uint32_t n_images = 0, added = 0;
    size_t first = 0, window = 0;                   // the window's first voxel in the grid, and its voxels
};

// one plane of sort keys per added image
struct frog_rank : frog_windowed {
    frog::DevBuf<uint32_t> d_keys;                  // n_images planes of `window` keys, in the order of the adds
};

// The taps of the three axes, and the scratch of the passes over a RANGE of whole planes (k_smooth.hip.h): the f32 values the
// x pass reads, and what the x and the y pass store.
struct SmoothWork {
    SmoothTaps taps[3];
    frog::DevBuf<float> d_raw;
    frog::DevBuf<double2> d_x, d_y;
};
constexpr size_t SMOOTH_VOXEL_BYTES = sizeof(float) + 2 * sizeof(double2);

// frog_glm_smooth's: the range an add evaluates, the window extended by the z radius and clipped at the grid's ends
struct SmoothPlan {
    bool on = false;
    size_t first = 0, count = 0;                    // the range's first voxel in the grid, and its voxels
    SmoothWork work;
};

// one plane of f32 values per added image, and the design of the linear model
struct frog_glm : frog_windowed {
    uint32_t p = 0;
    std::vector<double> design;                     // n_images x p
    frog::DevBuf<float> d_vals;                     // n_images planes of `window` values, in the order of the adds
    frog::DevBuf<double> d_design, d_table;         // d_table: the design rows of one launch's permutations, grown on demand
    SmoothPlan smooth;                              // frog_glm_smooth's; off at first
};

// n_components f32 per added image and window voxel, a voxel's components next to each other
struct frog_modes : frog_windowed {
    uint32_t components = 0;
    frog::DevBuf<float> d_vals;                     // n_images planes of `window` x components values, in the order of the adds
};

// what glm_fit_kernel stores besides the extrema: nothing, the bits of a frog_clusters or the levels of a frog_tfce
struct GlmStore {
    enum Kind { NONE, BITS, LEVELS } kind = NONE;
    GlmSink bits{};
    GlmLevelSink levels{};
};

// what the sinks of a permutation test hold alike (frog_clusters, frog_tfce): one slot per permutation, contrast and side for
// the whole grid, and which planes of it each permutation has received
struct frog_sink : frog_group {
    uint32_t n_perms = 0, n_contrasts = 0, sides = 1;
    CclGrid ccl{};
    size_t slots = 0;                               // n_perms * n_contrasts * sides
    uint32_t batch = 0;                             // the slots one launch labels: the workspace holds that many
    std::vector<uint8_t> received;                  // [perm * nz + z]: the plane has been written for the permutation's slots
    GlmStore store;                                 // the sink as the fit kernel sees it; `first` and `perm0` are a launch's
};

// the supra-threshold voxels of every permutation, contrast and side of a permutation test on one grid, as bit masks of
// ccl.words words, and the workspace that labels their connected components
struct frog_clusters : frog_sink {
    frog::DevBuf<uint32_t> d_bits, d_parent, d_extent, d_stats;
};

// the levels of every permutation, contrast and side of a permutation test on one grid, one byte per voxel and `stride`
// bytes per slot (k_tfce.hip.h), and the workspace that enhances a batch of them
struct TfceWork {
    frog::DevBuf<uint32_t> d_bits, d_parent, d_extent;      // of `batch` slots: k_ccl.hip.h's masks and workspace
    frog::DevBuf<double> d_acc;                             // of `batch` slots: one sum per voxel
};
struct TfceParams {
    float dh = 0;
    bool root = true;                               // E == 0.5
    double weight[256] = {};                        // w_k; weight[0] is not used
};
struct frog_tfce : frog_sink {
    TfceParams par;
    size_t stride = 0;
    frog::DevBuf<uint8_t> d_levels;
    frog::DevBuf<uint32_t> d_top, d_best;           // per slot: the highest level, the bits of the largest tfce
    TfceWork work;
};

// The label table of frog_labels, frog_wlabels (and through it frog_jlabels) and frog_staple: the device hash map in which
// the adds' collect kernels number the label values they meet, the values that are accepted so far, and after finish the
// sorted table.  The labels_* functions below work on it.
struct LabelTable {
    uint32_t max_labels = 0;
    bool finished = false;
    LabelMap map{};                                 // device pointers into the four buffers below
    frog::DevBuf<long long> d_keys, d_values;
    frog::DevBuf<uint32_t> d_index, d_state;
    std::vector<long long> known;                   // dense index -> value: the labels of the accepted volumes
    // after finish: the table in ascending order of the values
    std::vector<long long> values;
    frog::DevBuf<long long> d_sorted_values;
};

// vote counts of a group's label maps on one grid
struct frog_labels : frog_group, LabelTable {
    uint32_t n_images = 0, added = 0;
    std::deque<frog::DevBuf<uint16_t>> planes;      // one per known label; growth never copies counts
    frog::DevBuf<uint16_t *> d_planes;              // dense index -> plane
    // after finish (labels without a vote dropped from the table)
    std::vector<uint32_t> dense;                    // table position -> dense index
    std::vector<uint64_t> voxels, pairs;
    frog::DevBuf<uint16_t *> d_sorted_planes;
};

// weighted votes of a group of atlases for a target image on one grid
struct frog_wlabels : frog_group, LabelTable {
    uint32_t n_images = 0, added = 0, radius = 0, power = 0;
    float floor = 0;
    bool has_target = false;
    std::deque<frog::DevBuf<float>> planes;         // one f32 score plane per known label
    frog::DevBuf<float *> d_planes;                 // dense index -> plane
    frog::DevBuf<float> d_target, d_atlas;          // t and a on the grid, NaN where not valid
    frog::DevBuf<unsigned char> d_lsrc, d_lout;     // staging of the current label map / resliced label map
    // after finish
    std::vector<uint32_t> dense;                    // table position -> dense index
    frog::DevBuf<float *> d_sorted_planes;
};

// joint label fusion: frog_wlabels' target plane, label map and score planes, and what the adds leave for finish
struct frog_jlabels : frog_wlabels {
    uint32_t beta = 0;
    double alpha = 0;
    frog::DevBuf<float> d_atlases, d_weights;       // n_images planes each; d_weights only with keep_weights
    std::deque<frog::DevBuf<unsigned char>> label_maps;     // the added atlases' label maps on the grid, in their own types
    std::vector<int> ltypes;
    frog::DevBuf<const void *> d_label_maps;
    frog::DevBuf<int> d_ltypes;
};

// the dense label index of every image at every voxel of one grid, and the EM state of frog_staple_solve
struct frog_staple : frog_group, LabelTable {
    uint32_t n_images = 0, added = 0;
    bool solved = false;
    frog::DevBuf<uint8_t> d_D;                      // n_images planes: before finish the adds' indices, after it D[i][v]
    // after finish
    frog::DevBuf<uint8_t> d_active;
    frog::DevBuf<uint32_t> d_q;                     // L planes
    frog::DevBuf<double> d_theta, d_prior;
    frog::DevBuf<unsigned long long> d_S, d_T, d_word;      // d_word: c[l] (L words), then the change maximum
    // after solve: what frog_staple_performance returns
    std::vector<double> theta, prior;
    std::vector<uint64_t> sums, totals;
};

// the reference's distance maps, and what an add needs of the reference and of the current image
struct frog_surface : frog_group {
    uint32_t percentile = 95;
    std::vector<long long> values;                  // ascending
    frog::DevBuf<long long> d_values;
    frog::DevBuf<uint16_t> d_ref_idx, d_idx;        // dense label index of the reference / of the current image
    frog::DevBuf<uint8_t> d_ref_surf, d_surf;       // their surface masks
    frog::DevBuf<uint32_t> d_maps;                  // D_B: one grid-sized map per value
    std::vector<uint32_t> ref_bounds;               // per value EDT_BOUND_WORDS words: the box of B and n_b
    frog::DevBuf<uint32_t> d_bounds, d_any, d_largest;
    frog::DevBuf<unsigned long long> d_sum, d_count;
    frog::DevBuf<double> d_g1, d_g2;                // the passes' planes, grown to the largest box
    frog::DevBuf<uint2> d_list;
};

// a triangle mesh on the device: what frog_isosurface_create extracted, where frog_isosurface_apply moves it
struct frog_isosurface {
    int device = 0;
    uint32_t n_vertices = 0, n_triangles = 0;
    frog::DevBuf<float> d_xyz;                      // 3 per vertex
    frog::DevBuf<uint32_t> d_triangles;             // 3 per triangle
};

namespace {

int fail(int code, const std::string &msg) { frog::set_last_error(msg); return code; }

// a failed HIP call: a refused device allocation is FROG_E_NOMEM from every entry point, as frog_create reports it
int hip_fail(const std::string &what, hipError_t e)
{
    return fail(e == hipErrorOutOfMemory ? FROG_E_NOMEM : FROG_E_HIP, what + ": " + hipGetErrorString(e));
}

#define KCHECK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return hip_fail(#expr, e_);                                    \
    } while (0)

// the device of a new handle, made current
int select_device(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FROG_E_NODEVICE, "no HIP device: no CPU fallback");
    if (device < 0 || device >= count) return fail(FROG_E_INVALID, "bad device index");
    KCHECK(hipSetDevice(device));
    return FROG_OK;
}

bool integer_voxel_type(int dtype) { return dtype >= FROG_V_U8 && dtype <= FROG_V_I32; }

// f(S()) with S the C type of an integer FROG_V_* value, which the caller has checked with integer_voxel_type
template <class F>
int with_integer_voxel_type(int dtype, F f)
{
    switch (dtype) {
    case FROG_V_U8: return f(uint8_t());
    case FROG_V_I8: return f(int8_t());
    case FROG_V_U16: return f(uint16_t());
    case FROG_V_I16: return f(int16_t());
    case FROG_V_U32: return f(uint32_t());
    default: return f(int32_t());
    }
}

// f(S()) with S the C type of a FROG_V_* value
template <class F>
int with_voxel_type(int dtype, F f)
{
    if (integer_voxel_type(dtype)) return with_integer_voxel_type(dtype, f);
    switch (dtype) {
    case FROG_V_F32: return f(float());
    case FROG_V_F64: return f(double());
    default: return fail(FROG_E_INVALID, "unknown scalar type");
    }
}

size_t voxel_count(const frog_volume *v) { return (size_t)v->dims[0] * v->dims[1] * v->dims[2]; }

// Every launch in this file goes through chunked_launch: one work-item per element of [0, total), 256 per block, at most
// 2^31 work-items per launch.  A dispatch packet's grid is 32-bit WORK-ITEMS per dimension; a larger 1-D launch returns no
// error and the work-items past 2^32 never run.  launch(blocks, base) issues one chunk, whose kernel adds
// `base` (a multiple of 256) to its own index and bound-checks against the total.
constexpr size_t LAUNCH_BLOCK = 256;

size_t launch_max()
{
    // (test hook: FROG_CHAIN_LAUNCH_MAX=n, at most n work-items per launch, rounded down to whole blocks)
    static const size_t m = [] {
        const size_t cap = (size_t)1 << 31;
        const char *s = getenv("FROG_CHAIN_LAUNCH_MAX");
        const long long v = s ? atoll(s) : 0;
        return v > 0 ? std::max(LAUNCH_BLOCK, std::min(cap, (size_t)v) / LAUNCH_BLOCK * LAUNCH_BLOCK) : cap;
    }();
    return m;
}

template <class Launch>
hipError_t chunked_launch(size_t total, Launch launch)
{
    const size_t step = launch_max();
    for (size_t base = 0; base < total; base += step) {
        const size_t n = std::min(step, total - base);
        launch((unsigned)((n + LAUNCH_BLOCK - 1) / LAUNCH_BLOCK), base);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

NodeGrid node_grid(const double origin[3], const double spacing[3], const uint32_t dims[3])
{
    NodeGrid g;
    for (int k = 0; k < 3; k++) { g.origin[k] = origin[k]; g.spacing[k] = spacing[k]; g.dims[k] = dims[k]; }
    return g;
}

// frog_chain_sample's device buffers hold one slab of the grid: whole launches (chunked_launch's step), at most
// SAMPLE_SLAB_LAUNCHES of them, within SAMPLE_SLAB_BYTES and half of the free device memory; where one launch does not fit,
// a part of one.  Each slab is computed, then copied to its place in the host arrays.
constexpr size_t SAMPLE_SLAB_BYTES = (size_t)1 << 30;
constexpr size_t SAMPLE_SLAB_LAUNCHES = 4;

template <class T>
int sample_typed(frog_chain *c, const NodeGrid &grid, size_t total, T *displacement, T *determinant)
{
    const size_t per_node = ((displacement ? 3 : 0) + (determinant ? 1 : 0)) * sizeof(T);
    size_t free_bytes = 0, device_bytes = 0;
    KCHECK(hipMemGetInfo(&free_bytes, &device_bytes));
    const size_t step = launch_max();
    const size_t fit = std::max(LAUNCH_BLOCK, std::min(free_bytes / 2, SAMPLE_SLAB_BYTES) / per_node / LAUNCH_BLOCK * LAUNCH_BLOCK);
    size_t slab = fit >= step ? std::min(fit / step, SAMPLE_SLAB_LAUNCHES) * step : fit;
    slab = std::min(slab, (total + LAUNCH_BLOCK - 1) / LAUNCH_BLOCK * LAUNCH_BLOCK);
    frog::DevBuf<T> d_disp, d_det;
    if (displacement) KCHECK(d_disp.alloc(3 * slab));
    if (determinant) KCHECK(d_det.alloc(slab));
    const auto kernel = displacement && determinant ? chain_sample_kernel<true, true, T>
                      : displacement ? chain_sample_kernel<true, false, T> : chain_sample_kernel<false, true, T>;
    hipError_t e = hipSuccess;
    for (size_t first = 0; first < total && e == hipSuccess; first += slab) {
        const size_t count = std::min(slab, total - first);
        e = chunked_launch(count, [&](unsigned blocks, size_t base) {
            kernel<<<blocks, LAUNCH_BLOCK>>>(first, base, count, c->d_links.p, (int)c->h_links.size(), grid, d_disp.p, d_det.p);
        });
        if (e == hipSuccess && displacement) e = hipMemcpy(displacement + 3 * first, d_disp.p, 3 * count * sizeof(T), hipMemcpyDeviceToHost);
        if (e == hipSuccess && determinant) e = hipMemcpy(determinant + first, d_det.p, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return hip_fail("frog_chain_sample", e);
    return FROG_OK;
}

ResliceGrid reslice_grid(const frog_volume *src, const frog_volume *out, int interpolation, double background)
{
    ResliceGrid g;
    g.sx = (int)src->dims[0]; g.sy = (int)src->dims[1]; g.sz = (int)src->dims[2];
    for (int k = 0; k < 3; k++) { g.so[k] = src->origin[k]; g.ss[k] = src->spacing[k]; }
    g.out = node_grid(out->origin, out->spacing, out->dims);
    g.linear = interpolation != 0;
    g.background = background;
    return g;
}

template <class S>
int reslice_typed(frog_chain *c, const frog_volume *src, frog_volume *out, int interpolation, double background)
{
    const size_t n_src = voxel_count(src), n_out = voxel_count(out);
    frog::DevBuf<S> d_src, d_out;
    KCHECK(d_src.alloc(n_src));
    KCHECK(d_out.alloc(n_out));
    hipError_t e = hipMemcpy(d_src.p, src->data, n_src * sizeof(S), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const ResliceGrid g = reslice_grid(src, out, interpolation, background);
        e = chunked_launch(n_out, [&](unsigned blocks, size_t base) {
            reslice_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src.p, g, d_out.p);
        });
    }
    if (e == hipSuccess) e = hipMemcpy(out->data, d_out.p, n_out * sizeof(S), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_chain_reslice", e);
    return FROG_OK;
}

// The geometry of a mask for the kernels: zeros without one.
MaskGrid mask_grid(const frog_volume *mask)
{
    MaskGrid mg{};
    if (mask) {
        mg.sx = (int)mask->dims[0]; mg.sy = (int)mask->dims[1]; mg.sz = (int)mask->dims[2];
        for (int k = 0; k < 3; k++) { mg.so[k] = mask->origin[k]; mg.ss[k] = mask->spacing[k]; }
    }
    return mg;
}

// ---- what the adds of frog_average, frog_cover (and its score) and frog_labels share -----------------------------------------

// A volume whose voxels a chain's positions can be turned into: dimensions an int holds, spacings that divide.
bool chain_samples(const frog_volume *v)
{
    for (int k = 0; k < 3; k++)
        if (v->dims[k] > 0x7FFFFFFFu || !(v->spacing[k] != 0.0)) return false;
    return true;
}

bool grid_sized(const frog_group *a, const frog_volume *v)
{
    return v->dims[0] == a->grid.dims[0] && v->dims[1] == a->grid.dims[1] && v->dims[2] == a->grid.dims[2];
}

// What every add, and the score, refuses alike, in this order: a chain on another device than the accumulator's; an empty
// source; with a chain a source it cannot sample, without one a source that is not grid-sized; a resliced volume (null: none
// asked for, and the score has none) that is not grid-sized; one without voxels or of another type than the source's.
// `where`, the entry point, goes in front of the messages that name it.
int add_inputs(const char *where, const frog_group *a, const frog_chain *c, const frog_volume *src, const frog_volume *resliced)
{
    const std::string w = std::string(where) + ": ";
    if (c && c->device != a->device) return fail(FROG_E_INVALID, w + "chain and accumulator on different devices");
    if (!voxel_count(src)) return fail(FROG_E_INVALID, "empty volume");
    if (c && !chain_samples(src)) return fail(FROG_E_INVALID, "bad source geometry");
    if (!c && !grid_sized(a, src)) return fail(FROG_E_INVALID, w + "volume dimensions differ from the grid's");
    if (resliced && !grid_sized(a, resliced)) return fail(FROG_E_INVALID, w + "resliced volume is not grid-sized");
    if (resliced && (!resliced->data || resliced->dtype != src->dtype)) return fail(FROG_E_INVALID, w + "resliced volume must have the source's type");
    return FROG_OK;
}

// The staging step of an add: a->d_src grown and filled with the source, a->d_out grown to a grid-sized volume of S where
// `want_out` says the kernel stores the resliced volume; *g receives the geometry the kernels take.
template <class S>
int stage_source(const char *where, frog_group *a, const frog_volume *src, bool want_out, int interpolation, double background, ResliceGrid *g)
{
    const size_t n_src = voxel_count(src);
    KCHECK(a->d_src.alloc(n_src * sizeof(S)));
    if (want_out) KCHECK(a->d_out.alloc(a->total * sizeof(S)));
    const hipError_t e = hipMemcpy(a->d_src.p, src->data, n_src * sizeof(S), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(where, e);
    *g = reslice_grid(src, &a->grid, interpolation, background);
    return FROG_OK;
}

// A volume an add hands back on the grid, after launches that ended with `e`, where one is asked for: the `bytes` the chain
// kernel stored at d_on_grid; without a chain the source itself.
hipError_t copy_resliced(const frog_chain *c, const frog_volume *src, frog_volume *resliced, const void *d_on_grid, size_t bytes, hipError_t e)
{
    if (e == hipSuccess && resliced) {
        if (c) e = hipMemcpy(resliced->data, d_on_grid, bytes, hipMemcpyDeviceToHost);
        else std::memcpy(resliced->data, src->data, bytes);
    }
    return e;
}

// The return step of an add, after launches that ended with `e`: the resliced volume (in a->d_out), then the stream drained.
template <class S>
int return_resliced(const char *where, frog_group *a, const frog_chain *c, const frog_volume *src, frog_volume *resliced, hipError_t e)
{
    e = copy_resliced(c, src, resliced, a->d_out.p, a->total * sizeof(S), e);
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) return hip_fail(where, e);
    return FROG_OK;
}

template <class S>
int average_add_typed(frog_average *a, frog_chain *c, const frog_volume *src, int interpolation, double background, frog_volume *resliced)
{
    ResliceGrid g;
    if (int rc = stage_source<S>("frog_average_add", a, src, c && resliced, interpolation, background, &g)) return rc;
    const float n = (float)a->n_images;
    const S *d_src = (const S *)a->d_src.p;
    S *d_out = (S *)a->d_out.p;
    const hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        if (c)
            reslice_accumulate_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, n,
                                                                   a->d_avg.p, a->d_sq.p, resliced ? d_out : nullptr);
        else
            identity_accumulate_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, d_src, a->total, n, a->d_avg.p, a->d_sq.p);
    });
    return return_resliced<S>("frog_average_add", a, c, src, resliced, e);
}

// the masked accumulators' part of the staging step: the mask of an add or a score, which cover_mask left as bytes in
// a->h_mask, on the device; a null pointer without one
int cover_stage_mask(const char *where, frog_masked *a, const frog_volume *mask, const uint8_t **d_mask)
{
    *d_mask = nullptr;
    if (!mask) return FROG_OK;
    const size_t n_mask = voxel_count(mask);
    KCHECK(a->d_mask.alloc(n_mask));
    const hipError_t e = hipMemcpy(a->d_mask.p, a->h_mask.data(), n_mask, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(where, e);
    *d_mask = a->d_mask.p;
    return FROG_OK;
}

template <class S>
int cover_add_typed(frog_cover *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background,
                    frog_volume *resliced)
{
    ResliceGrid g;
    const uint8_t *d_mask;
    if (int rc = stage_source<S>("frog_cover_add", a, src, c && resliced, interpolation, background, &g)) return rc;
    if (int rc = cover_stage_mask("frog_cover_add", a, mask, &d_mask)) return rc;
    const MaskGrid mg = mask_grid(mask);
    const S *d_src = (const S *)a->d_src.p;
    S *d_out = (S *)a->d_out.p;
    const hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        if (c)
            cover_reslice_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, d_mask, mg,
                                                              a->d_mean.p, a->d_m2.p, a->d_count.p, resliced ? d_out : nullptr);
        else
            cover_identity_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, d_src, d_mask, a->total, a->d_mean.p, a->d_m2.p, a->d_count.p);
    });
    return return_resliced<S>("frog_cover_add", a, c, src, resliced, e);
}

template <class S>
int cover_score_typed(frog_cover *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background,
                      const ScoreParams &sp, frog_score_sums *sums, uint64_t *histogram)
{
    const size_t tiles = (a->total + SCORE_TILE - 1) / SCORE_TILE, cells = (size_t)sp.bins * sp.bins;
    frog::DevBuf<ScorePartial> d_partials;
    frog::DevBuf<unsigned long long> d_hist;
    KCHECK(d_partials.alloc(tiles));
    if (cells) KCHECK(d_hist.alloc(cells));
    std::vector<ScorePartial> partials(tiles);
    ResliceGrid g;
    const uint8_t *d_mask;
    if (int rc = stage_source<S>("frog_cover_score", a, src, false, interpolation, background, &g)) return rc;
    if (int rc = cover_stage_mask("frog_cover_score", a, mask, &d_mask)) return rc;
    const MaskGrid mg = mask_grid(mask);
    const S *d_src = (const S *)a->d_src.p;
    hipError_t e = cells ? hipMemset(d_hist.p, 0, cells * sizeof(unsigned long long)) : hipSuccess;
    if (e == hipSuccess) {
        const size_t lds = cells * sizeof(uint32_t);
        // one block per tile: the work-items are the tiles padded to whole blocks, so a launch chunk never splits a tile
        e = chunked_launch(tiles * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) {
            if (c)
                cover_score_kernel<S><<<blocks, LAUNCH_BLOCK, lds>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, d_mask, mg,
                                                                     a->d_mean.p, a->d_count.p, sp, d_partials.p, d_hist.p);
            else
                cover_score_identity_kernel<S><<<blocks, LAUNCH_BLOCK, lds>>>(base, d_src, d_mask, a->total, a->d_mean.p, a->d_count.p, sp,
                                                                              d_partials.p, d_hist.p);
        });
    }
    if (e == hipSuccess) e = hipMemcpy(partials.data(), d_partials.p, tiles * sizeof(ScorePartial), hipMemcpyDeviceToHost);
    if (e == hipSuccess && cells) e = hipMemcpy(histogram, d_hist.p, cells * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_cover_score", e);
    // the last pass of the stated order: the tiles in ascending index, serially, f64 (this file is built with -ffp-contract=off)
    frog_score_sums t{};
    double s[6] = { 0, 0, 0, 0, 0, 0 };
    for (const ScorePartial &p : partials) {
        for (int q = 0; q < 6; q++) s[q] += p.s[q];
        t.n += p.n;
        t.n_nonfinite += p.n_nonfinite;
    }
    t.sx = s[0]; t.sy = s[1]; t.sxx = s[2]; t.syy = s[3]; t.sxy = s[4]; t.sad = s[5];
    *sums = t;
    return FROG_OK;
}

// the mask of an add or a score as bytes, value != 0, in a->h_mask
void cover_mask(frog_masked *a, const frog_volume *mask)
{
    with_integer_voxel_type(mask->dtype, [&](auto m) {
        const size_t n = voxel_count(mask);
        const decltype(m) *v = (const decltype(m) *)mask->data;
        a->h_mask.resize(n);
        for (size_t i = 0; i < n; i++) a->h_mask[i] = v[i] != 0;
        return FROG_OK;
    });
}

// what frog_cover_add, frog_cover_score and frog_rank_add refuse alike: add_inputs, then what concerns the mask
int cover_inputs(const char *where, const frog_masked *a, const frog_chain *c, const frog_volume *src, const frog_volume *mask,
                 const frog_volume *resliced)
{
    if (int rc = add_inputs(where, a, c, src, resliced)) return rc;
    if (!mask) return FROG_OK;
    const std::string w = std::string(where) + ": ";
    if (!mask->data) return fail(FROG_E_INVALID, w + "a mask without voxels");
    if (!integer_voxel_type(mask->dtype)) return fail(FROG_E_INVALID, w + "a mask has an integer type");
    if (!voxel_count(mask)) return fail(FROG_E_INVALID, "empty volume");
    if (c && !chain_samples(mask)) return fail(FROG_E_INVALID, "bad mask geometry");
    if (!c && !grid_sized(a, mask)) return fail(FROG_E_INVALID, w + "mask dimensions differ from the grid's");
    return FROG_OK;
}

// ---- the label table (LabelTable) of frog_labels, frog_staple, frog_wlabels and frog_jlabels ---------------------------------

// The device map rebuilt from the known labels alone (at creation: empty): how a refused volume's inserts are taken back.
hipError_t labels_reset_map(LabelTable *t)
{
    const size_t slots = (size_t)t->map.mask + 1;
    std::vector<long long> keys(slots, LABEL_EMPTY);
    std::vector<uint32_t> index(slots, 0);
    for (size_t i = 0; i < t->known.size(); i++) {
        uint32_t slot = label_slot(t->known[i], t->map.shift);
        while (keys[slot] != LABEL_EMPTY) slot = (slot + 1) & t->map.mask;            // load <= 1/2: a free slot exists
        keys[slot] = t->known[i];
        index[slot] = (uint32_t)i;
    }
    const uint32_t state[2] = { (uint32_t)t->known.size(), 0 };
    hipError_t e = hipMemcpy(t->d_keys.p, keys.data(), slots * sizeof(long long), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_index.p, index.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_state.p, state, sizeof state, hipMemcpyHostToDevice);
    return e;
}

// The empty device map of a new accumulator for max_labels labels: at least 16 slots, at least two per label.
int labels_new_map(LabelTable *t, uint32_t max_labels)
{
    t->max_labels = max_labels;
    int bits = 4;
    while (((size_t)1 << bits) < 2 * (size_t)max_labels) bits++;
    const size_t slots = (size_t)1 << bits;
    KCHECK(t->d_keys.alloc(slots));
    KCHECK(t->d_index.alloc(slots));
    KCHECK(t->d_values.alloc(max_labels));
    KCHECK(t->d_state.alloc(2));
    t->map = LabelMap{ t->d_keys.p, t->d_index.p, t->d_values.p, t->d_state.p, (uint32_t)(slots - 1), 64 - bits, max_labels };
    KCHECK(labels_reset_map(t));
    return FROG_OK;
}

// After an add's collect the map may hold values that `known` does not: every failure from there on takes them back, so
// the volume leaves no label behind.
int labels_refuse(LabelTable *t, int rc) { (void)labels_reset_map(t); return rc; }

// What follows the collect launches of `where`, which ended with `e`: the map's state read, and a volume refused whose
// labels do not fit the table.  *n_now: the labels the map holds now, the known ones first.
int labels_collected(const char *where, LabelTable *t, hipError_t e, size_t *n_now)
{
    uint32_t state[2] = { 0, 0 };
    if (e == hipSuccess) e = hipMemcpy(state, t->d_state.p, sizeof state, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return labels_refuse(t, hip_fail(where, e));
    if (state[1] || state[0] > t->max_labels)
        return labels_refuse(t, fail(FROG_E_INVALID, std::string(where) + ": more than max_labels = " + std::to_string(t->max_labels) + " distinct labels"));
    *n_now = state[0];
    return FROG_OK;
}

// the values of the labels the map holds beyond the known ones, in the order of their dense indices
hipError_t labels_fresh_values(const LabelTable *t, size_t n_now, std::vector<long long> &fresh)
{
    const size_t n_known = t->known.size();
    fresh.resize(n_now - n_known);
    if (fresh.empty()) return hipSuccess;
    return hipMemcpy(fresh.data(), t->d_values.p + n_known, fresh.size() * sizeof(long long), hipMemcpyDeviceToHost);
}

// The planes of the labels an add has found beyond those that had one: a zeroed plane of P each, the pointers behind
// d_planes, and then the labels known.  On a failure the new planes are gone again and `known` is as it was.
template <class P>
hipError_t labels_grow_planes(LabelTable *t, size_t total, size_t n_now, std::deque<frog::DevBuf<P>> &planes, P **d_planes)
{
    const size_t n_known = t->known.size();
    std::vector<long long> fresh;
    std::vector<P *> pointers;
    hipError_t e = labels_fresh_values(t, n_now, fresh);
    if (fresh.empty()) return e;
    for (size_t i = 0; i < fresh.size() && e == hipSuccess; i++) {
        planes.emplace_back();
        e = planes.back().alloc(total);
        if (e == hipSuccess) e = hipMemset(planes.back().p, 0, total * sizeof(P));
        pointers.push_back(planes.back().p);
    }
    if (e == hipSuccess) e = hipMemcpy(d_planes + n_known, pointers.data(), pointers.size() * sizeof(P *), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        while (planes.size() > n_known) planes.pop_back();
        return e;
    }
    t->known.insert(t->known.end(), fresh.begin(), fresh.end());
    return hipSuccess;
}

// The table of a finish: `order`, the dense indices of the labels that enter it, sorted by their values; those values in
// t->values and on the device.
int labels_sort(LabelTable *t, std::vector<uint32_t> &order)
{
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return t->known[x] < t->known[y]; });
    t->values.clear();
    for (const uint32_t i : order) t->values.push_back(t->known[i]);
    KCHECK(t->d_sorted_values.alloc(order.size()));
    KCHECK(hipMemcpy(t->d_sorted_values.p, t->values.data(), order.size() * sizeof(long long), hipMemcpyHostToDevice));
    return FROG_OK;
}

// every known label in the order of the adds: what a finish that drops none hands to labels_sort
std::vector<uint32_t> labels_all(const LabelTable *t)
{
    std::vector<uint32_t> order(t->known.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
    return order;
}

// the planes of a sorted table's labels behind d_sorted_planes
template <class P>
int labels_sort_planes(const std::vector<uint32_t> &order, std::deque<frog::DevBuf<P>> &planes, frog::DevBuf<P *> &d_sorted_planes)
{
    std::vector<P *> sorted_planes;
    for (const uint32_t i : order) sorted_planes.push_back(planes[i].p);
    KCHECK(d_sorted_planes.alloc(order.size()));
    KCHECK(hipMemcpy(d_sorted_planes.p, sorted_planes.data(), order.size() * sizeof(P *), hipMemcpyHostToDevice));
    return FROG_OK;
}

// *l: the position of `value` in the sorted table; `where`: `tail` if it is not there
int labels_find(const char *where, const char *tail, const LabelTable *t, int64_t value, size_t *l)
{
    const auto it = std::lower_bound(t->values.begin(), t->values.end(), (long long)value);
    if (it == t->values.end() || *it != (long long)value) return fail(FROG_E_INVALID, std::string(where) + ": " + tail);
    *l = (size_t)(it - t->values.begin());
    return FROG_OK;
}

// every value of the table is a T
template <class T>
bool labels_fit(const LabelTable *t)
{
    for (const long long v : t->values)
        if (v < (long long)std::numeric_limits<T>::lowest() || v > (long long)std::numeric_limits<T>::max()) return false;
    return true;
}

// How every getter of a label accumulator opens: `given`, its arguments are all there; `ready`, the accumulator is past
// the call `after`, from which on the getter has something to give.
int labels_getter(const char *where, bool given, bool ready, const char *after)
{
    if (!given) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (!ready) return fail(FROG_E_INVALID, std::string(where) + ": before " + after);
    return FROG_OK;
}

// what the frog_*_values entry points give: the sorted table
int labels_values(const char *where, const LabelTable *t, const char *after, int64_t *values)
{
    if (int rc = labels_getter(where, t && values, t && t->finished, after)) return rc;
    for (size_t l = 0; l < t->values.size(); l++) values[l] = t->values[l];
    return FROG_OK;
}

// What the frog_*_fused entry points refuse alike, in this order, before the accumulator's device is made current: missing
// arguments, an accumulator that is not `ready` (past `after`), a fused map of a type that is no integer's or not grid-sized.
int fused_arguments(const char *where, const frog_group *a, bool ready, const char *after, const frog_volume *label, const float *second)
{
    const std::string w = std::string(where) + ": ";
    if (int rc = labels_getter(where, a && (label || second) && (!label || label->data), ready, after)) return rc;
    if (label) {
        if (!integer_voxel_type(label->dtype)) return fail(FROG_E_INVALID, w + "the fused map has an integer type");
        if (!grid_sized(a, label)) return fail(FROG_E_INVALID, w + "the fused map is not grid-sized");
    }
    KCHECK(hipSetDevice(a->device));
    return FROG_OK;
}

// A fused output of type T: the fused map and its f32 companion (agreement or confidence), each only where asked for, on the
// device; launch(blocks, base, d_label, d_second) for the chunks of the grid; the copies back.
template <class T, class Launch>
int fused_output(const char *where, const frog_group *a, frog_volume *label, float *second, Launch launch)
{
    frog::DevBuf<T> d_label;
    frog::DevBuf<float> d_second;
    if (label) KCHECK(d_label.alloc(a->total));
    if (second) KCHECK(d_second.alloc(a->total));
    hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) { launch(blocks, base, d_label.p, d_second.p); });
    if (e == hipSuccess && label) e = hipMemcpy(label->data, d_label.p, a->total * sizeof(T), hipMemcpyDeviceToHost);
    if (e == hipSuccess && second) e = hipMemcpy(second, d_second.p, a->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(where, e);
    return FROG_OK;
}

// A probability output: the accumulator's device made current, one f32 plane of the grid on it, launch(blocks, base, d_p) for
// the chunks of the grid, the copy back.
template <class Launch>
int probability_output(const char *where, const frog_group *a, float *p, Launch launch)
{
    KCHECK(hipSetDevice(a->device));
    frog::DevBuf<float> d_p;
    KCHECK(d_p.alloc(a->total));
    hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) { launch(blocks, base, d_p.p); });
    if (e == hipSuccess) e = hipMemcpy(p, d_p.p, a->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(where, e);
    return FROG_OK;
}

// The collect step of frog_labels_add and frog_staple_add for a source of type S: the source staged and its labels -- with a
// chain the resliced ones, which the kernel leaves in a->d_out -- numbered in the table's map.  *d_labels: those labels on the
// grid; *n_now as labels_collected gives it.
template <class S>
int labels_collect(const char *where, frog_group *a, LabelTable *t, frog_chain *c, const frog_volume *src, double background,
                   const S **d_labels, size_t *n_now)
{
    ResliceGrid g;
    if (int rc = stage_source<S>(where, a, src, c != nullptr, 0, background, &g)) return rc;
    const S *d_src = (const S *)a->d_src.p;
    S *d_out = (S *)a->d_out.p;                     // with a chain the votes are read from the resliced labels
    *d_labels = c ? d_out : d_src;
    const hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        if (c)
            labels_collect_kernel<S, true><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, a->total, d_out, t->map);
        else
            labels_collect_kernel<S, false><<<blocks, LAUNCH_BLOCK>>>(base, nullptr, 0, d_src, g, a->total, nullptr, t->map);
    });
    return labels_collected(where, t, e, n_now);
}

template <class S>
int labels_add_typed(frog_labels *a, frog_chain *c, const frog_volume *src, double background, frog_volume *resliced)
{
    const S *d_labels;
    size_t n_now;
    if (int rc = labels_collect<S>("frog_labels_add", a, a, c, src, background, &d_labels, &n_now)) return rc;
    hipError_t e = labels_grow_planes<uint16_t>(a, a->total, n_now, a->planes, a->d_planes.p);
    if (e != hipSuccess) return labels_refuse(a, hip_fail("frog_labels_add", e));
    e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        labels_vote_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, d_labels, a->total, a->map, a->d_planes.p, (uint32_t)n_now);
    });
    return return_resliced<S>("frog_labels_add", a, c, src, resliced, e);
}

// the tiles of wlabels_vote_kernel over the accumulator's grid
WlabelsTiles wlabels_tiles(const frog_wlabels *a)
{
    WlabelsTiles w;
    w.nx = a->grid.dims[0]; w.ny = a->grid.dims[1]; w.nz = a->grid.dims[2];
    w.tx = (w.nx + WL_TX - 1) / WL_TX;
    w.ty = (w.ny + WL_TY - 1) / WL_TY;
    w.tiles = (size_t)w.tx * w.ty * ((w.nz + WL_TZ - 1) / WL_TZ);
    return w;
}

template <class S>
int wlabels_target_typed(const char *where, frog_wlabels *a, frog_chain *c, const frog_volume *src, int interpolation, double background,
                         frog_volume *resliced)
{
    ResliceGrid g;
    if (int rc = stage_source<S>(where, a, src, c && resliced, interpolation, background, &g)) return rc;
    const S *d_src = (const S *)a->d_src.p;
    S *d_out = resliced ? (S *)a->d_out.p : nullptr;
    const hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        if (c)
            wlabels_collect_kernel<S, true, false><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, nullptr, 0, g,
                                                                             a->total, a->d_target.p, d_out, nullptr, a->map);
        else
            wlabels_collect_kernel<S, false, false><<<blocks, LAUNCH_BLOCK>>>(base, nullptr, 0, d_src, g, nullptr, 0, g, a->total, a->d_target.p,
                                                                              nullptr, nullptr, a->map);
    });
    return return_resliced<S>(where, a, c, src, resliced, e);
}

// The collect step of frog_wlabels_add and frog_jlabels_add for an image of type S (the label map's type is a run-time
// argument of the kernels), after the caller has staged the image (g) and its label map (at d_lsrc): the atlas on the grid
// into `plane`, with a chain its label map on the grid into d_on_grid and, if `want_image`, the image into a->d_out; the
// labels numbered in the table's map, and a score plane for every new one.
template <class S>
int wlabels_collect(const char *where, frog_wlabels *a, frog_chain *c, const ResliceGrid &g, const frog_volume *labels, double label_background,
                    const void *d_lsrc, bool want_image, float *plane, void *d_on_grid)
{
    const ResliceGrid lg = reslice_grid(labels, &a->grid, 0, label_background);
    const int ltype = labels->dtype;
    const S *d_src = (const S *)a->d_src.p;
    S *d_out = want_image ? (S *)a->d_out.p : nullptr;
    hipError_t e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        if (c)
            wlabels_collect_kernel<S, true, true><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, d_lsrc, ltype, lg,
                                                                            a->total, plane, d_out, d_on_grid, a->map);
        else
            wlabels_collect_kernel<S, false, true><<<blocks, LAUNCH_BLOCK>>>(base, nullptr, 0, d_src, g, d_lsrc, ltype, lg, a->total, plane,
                                                                             nullptr, nullptr, a->map);
    });
    size_t n_now;
    if (int rc = labels_collected(where, a, e, &n_now)) return rc;
    e = labels_grow_planes<float>(a, a->total, n_now, a->planes, a->d_planes.p);
    if (e != hipSuccess) return labels_refuse(a, hip_fail(where, e));
    return FROG_OK;
}

template <class S>
int wlabels_add_typed(frog_wlabels *a, frog_chain *c, const frog_volume *image, const frog_volume *labels, int interpolation,
                      double image_background, double label_background, frog_volume *resliced_image, frog_volume *resliced_labels)
{
    ResliceGrid g;
    if (int rc = stage_source<S>("frog_wlabels_add", a, image, c && resliced_image, interpolation, image_background, &g)) return rc;
    const size_t label_bytes = frog_volume_voxel_bytes(labels->dtype), n_labels_src = voxel_count(labels);
    KCHECK(a->d_lsrc.alloc(n_labels_src * label_bytes));
    if (c) KCHECK(a->d_lout.alloc(a->total * label_bytes));
    KCHECK(hipMemcpy(a->d_lsrc.p, labels->data, n_labels_src * label_bytes, hipMemcpyHostToDevice));
    if (int rc = wlabels_collect<S>("frog_wlabels_add", a, c, g, labels, label_background, a->d_lsrc.p, resliced_image != nullptr, a->d_atlas.p,
                                    a->d_lout.p))
        return rc;
    const void *d_labels = c ? a->d_lout.p : a->d_lsrc.p;      // with a chain the votes are read from the resliced labels
    const int ltype = labels->dtype;
    const uint32_t n_now = (uint32_t)a->known.size();
    const WlabelsTiles w = wlabels_tiles(a);
    // one block per tile: the work-items are the tiles padded to whole blocks, so a launch chunk never splits a tile
    hipError_t e = chunked_launch(w.tiles * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) {
#define WLABELS_VOTE(R) wlabels_vote_kernel<R><<<blocks, LAUNCH_BLOCK>>>(base, a->d_target.p, a->d_atlas.p, d_labels, ltype, w, a->power, a->floor, \
                                                                        a->map, a->d_planes.p, n_now)
        switch (a->radius) {
        case 1: WLABELS_VOTE(1); break;
        case 2: WLABELS_VOTE(2); break;
        case 3: WLABELS_VOTE(3); break;
        default: WLABELS_VOTE(4); break;
        }
#undef WLABELS_VOTE
    });
    e = copy_resliced(c, labels, resliced_labels, a->d_lout.p, a->total * label_bytes, e);
    return return_resliced<S>("frog_wlabels_add", a, c, image, resliced_image, e);
}

// An add of frog_jlabels: the collect step into the atlas' own plane and label map, which stay for finish.
template <class S>
int jlabels_add_typed(frog_jlabels *a, frog_chain *c, const frog_volume *image, const frog_volume *labels, int interpolation,
                      double image_background, double label_background, frog_volume *resliced_image, frog_volume *resliced_labels)
{
    ResliceGrid g;
    if (int rc = stage_source<S>("frog_jlabels_add", a, image, c && resliced_image, interpolation, image_background, &g)) return rc;
    const size_t label_bytes = frog_volume_voxel_bytes(labels->dtype), n_labels_src = voxel_count(labels);
    frog::DevBuf<unsigned char> on_grid;
    KCHECK(on_grid.alloc(a->total * label_bytes));
    if (c) KCHECK(a->d_lsrc.alloc(n_labels_src * label_bytes));
    unsigned char *const d_lsrc = c ? a->d_lsrc.p : on_grid.p;             // without a chain the map is on the grid as it is
    KCHECK(hipMemcpy(d_lsrc, labels->data, n_labels_src * label_bytes, hipMemcpyHostToDevice));
    float *const plane = a->d_atlases.p + (size_t)a->added * a->total;
    if (int rc = wlabels_collect<S>("frog_jlabels_add", a, c, g, labels, label_background, d_lsrc, resliced_image != nullptr, plane, on_grid.p))
        return rc;
    const hipError_t e = copy_resliced(c, labels, resliced_labels, on_grid.p, a->total * label_bytes, hipSuccess);
    const int rc = return_resliced<S>("frog_jlabels_add", a, c, image, resliced_image, e);
    if (rc != FROG_OK) return rc;
    a->label_maps.emplace_back();
    a->label_maps.back().swap(on_grid);
    a->ltypes.push_back(labels->dtype);
    return FROG_OK;
}

// finish of frog_jlabels: the solve and the votes of every voxel (k_joint.hip.h)
int jlabels_solve(frog_jlabels *a)
{
    const int n = (int)a->n_images, radius = (int)a->radius;
    std::vector<const void *> maps;
    for (const auto &m : a->label_maps) maps.push_back(m.p);
    KCHECK(a->d_label_maps.alloc(maps.size()));
    KCHECK(a->d_ltypes.alloc(maps.size()));
    KCHECK(hipMemcpy(a->d_label_maps.p, maps.data(), maps.size() * sizeof(const void *), hipMemcpyHostToDevice));
    KCHECK(hipMemcpy(a->d_ltypes.p, a->ltypes.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice));
    if (a->d_weights.p) KCHECK(hipMemset(a->d_weights.p, 0, (size_t)n * a->total * sizeof(float)));
    JointArgs j{};
    j.target = a->d_target.p; j.atlases = a->d_atlases.p; j.labels = a->d_label_maps.p; j.ltypes = a->d_ltypes.p;
    j.weights = a->d_weights.p; j.planes = a->d_planes.p; j.n_planes = (uint32_t)a->known.size(); j.map = a->map;
    j.total = a->total;
    j.nx = a->grid.dims[0]; j.ny = a->grid.dims[1]; j.nz = a->grid.dims[2];
    j.runs = (j.nx + JL_RUN - 1) / JL_RUN;
    j.tiles = (size_t)j.runs * j.ny * j.nz;
    j.n = n; j.radius = radius; j.beta = (int)a->beta; j.alpha = a->alpha;
    // lanes per voxel and pairs per lane: the smallest that hold the n (n + 1) / 2 pairs and the n + 1 planes of the statistics
    const int pairs = n * (n + 1) / 2;
    const int lanes = n <= 10 ? 32 : 64, ppl = pairs <= 128 ? 2 : pairs <= 256 ? 4 : pairs <= 384 ? 6 : 9;
    const size_t scratch = (size_t)(64 / lanes) * joint_group_doubles(n, radius) * sizeof(double);
    const size_t staged = scratch + joint_staged_floats(n, radius) * sizeof(float);
    j.staged = staged <= JL_LDS_BUDGET;
    const size_t lds = j.staged ? staged : scratch;
    // one block of 64 threads per tile: the work-items are the tiles times LAUNCH_BLOCK, so a launch chunk never splits a tile
    hipError_t e = chunked_launch(j.tiles * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) {
        if (lanes == 32) jlabels_solve_kernel<32, 2><<<blocks, 64, lds>>>(base, j);
        else if (ppl == 2) jlabels_solve_kernel<64, 2><<<blocks, 64, lds>>>(base, j);
        else if (ppl == 4) jlabels_solve_kernel<64, 4><<<blocks, 64, lds>>>(base, j);
        else if (ppl == 6) jlabels_solve_kernel<64, 6><<<blocks, 64, lds>>>(base, j);
        else jlabels_solve_kernel<64, 9><<<blocks, 64, lds>>>(base, j);
    });
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("frog_jlabels_finish", e);
    return FROG_OK;
}

// The opening of every accumulator's create: what it refuses without asking for a device, and the grid's voxels.  The
// accumulator's own argument checks follow, then group_new.
int group_arguments(const char *where, const frog_volume *grid, const void *out, size_t *total)
{
    if (!grid || !out) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    *total = voxel_count(grid);
    if (!*total) return fail(FROG_E_INVALID, "empty grid");
    // one thread per voxel, 256 per block: a grid above 2^31 voxels is refused here rather than launched
    if (*total > ((size_t)1 << 31)) return fail(FROG_E_INVALID, "grid above 2^31 voxels");
    return FROG_OK;
}

// an accumulator A on `device`, made current, that holds the grid and nothing else yet
template <class A>
int group_new(const frog_volume *grid, size_t total, int device, std::unique_ptr<A> &a)
{
    if (int rc = select_device(device)) return rc;
    a.reset(new (std::nothrow) A);
    if (!a) return fail(FROG_E_NOMEM, "out of host memory");
    a->device = device;
    a->grid = *grid;
    a->grid.data = nullptr;
    a->total = total;
    return FROG_OK;
}

template <class A>
void group_destroy(A *a)
{
    if (!a) return;
    (void)hipSetDevice(a->device);
    delete a;
}

// ---- the windowed plane store (frog_windowed) of frog_rank and frog_glm ------------------------------------------------------

// A new accumulator A with the window of n_planes z-planes from first_plane on, after the create's own argument checks.
template <class A>
int windowed_new(const char *where, const frog_volume *grid, size_t total, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, int device,
                 std::unique_ptr<A> &a)
{
    if (!n_planes || first_plane >= grid->dims[2] || n_planes > grid->dims[2] - first_plane)
        return fail(FROG_E_INVALID, std::string(where) + ": the window lies outside the grid or is empty");
    if (int rc = group_new(grid, total, device, a)) return rc;
    const size_t plane = (size_t)grid->dims[0] * grid->dims[1];
    a->n_images = n_images;
    a->first = plane * first_plane;
    a->window = plane * n_planes;
    return FROG_OK;
}

// An add for a source of type S: cover_add_typed with the store of Entry (RankEntry: a key, GlmEntry: an f32) in place of the
// update, over the window, into the image's plane.
template <class S, class Entry>
int windowed_add_typed(const char *where, frog_windowed *a, size_t first, size_t window, typename Entry::type *plane, frog_chain *c,
                       const frog_volume *src, const frog_volume *mask, int interpolation, double background)
{
    ResliceGrid g;
    const uint8_t *d_mask;
    if (int rc = stage_source<S>(where, a, src, false, interpolation, background, &g)) return rc;
    if (int rc = cover_stage_mask(where, a, mask, &d_mask)) return rc;
    const MaskGrid mg = mask_grid(mask);
    const S *d_src = (const S *)a->d_src.p;
    const hipError_t e = chunked_launch(window, [&](unsigned blocks, size_t base) {
        if (c)
            window_reslice_kernel<S, Entry><<<blocks, LAUNCH_BLOCK>>>(base, first, window, c->d_links.p, (int)c->h_links.size(), d_src, g, d_mask, mg, plane);
        else
            window_identity_kernel<S, Entry><<<blocks, LAUNCH_BLOCK>>>(base, first, window, d_src, d_mask, plane);
    });
    return return_resliced<S>(where, a, c, src, nullptr, e);
}

// frog_rank_add and frog_glm_add: `planes` is the accumulator's store, n_images planes of the window (null with a null a).
// With `range` the same kernels store the `range_count` voxels of the grid from `range_first` on there instead, and the add is
// not counted: the caller has more to do (frog_glm_add with smoothing).
template <class Entry>
int windowed_add(const char *where, frog_windowed *a, typename Entry::type *planes, frog_chain *c, const frog_volume *src, const frog_volume *mask,
                 int interpolation, double background, typename Entry::type *range = nullptr, size_t range_first = 0, size_t range_count = 0)
{
    if (!a || !src || !src->data || !frog_volume_voxel_bytes(src->dtype)) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (a->added >= a->n_images) return fail(FROG_E_INVALID, std::string(where) + ": more volumes than the accumulator was created for");
    if (int rc = cover_inputs(where, a, c, src, mask, nullptr)) return rc;
    if (mask) cover_mask(a, mask);
    KCHECK(hipSetDevice(a->device));
    const int rc = with_voxel_type(src->dtype, [&](auto s) {
        if (range) return windowed_add_typed<decltype(s), Entry>(where, a, range_first, range_count, range, c, src, mask, interpolation, background);
        return windowed_add_typed<decltype(s), Entry>(where, a, a->first, a->window, planes + (size_t)a->added * a->window, c, src, mask, interpolation,
                                                      background);
    });
    if (rc == FROG_OK && !range) a->added++;
    return rc;
}

// The finish kernels over the window: the register tier for up to RANK_REG_MAX planes, one work-item per voxel; above it the
// LDS tier, one block per tile of RANK_LDS_KEYS / P voxels.  P is the smallest of the padded sizes that holds the planes.
hipError_t rank_finish_launch(const frog_rank *a, const RankFinish &f)
{
    const uint32_t *keys = a->d_keys.p;
    auto reg = [&](auto kernel) {
        return chunked_launch(f.window, [&](unsigned blocks, size_t base) { kernel<<<blocks, LAUNCH_BLOCK>>>(base, keys, f); });
    };
    auto lds = [&](auto kernel, size_t padded) {
        const size_t per_tile = RANK_LDS_KEYS / padded, tiles = (f.window + per_tile - 1) / per_tile;
        return chunked_launch(tiles * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) { kernel<<<blocks, LAUNCH_BLOCK>>>(base, keys, f); });
    };
    if (f.n <= 8) return reg(rank_finish_reg_kernel<8>);
    if (f.n <= 16) return reg(rank_finish_reg_kernel<16>);
    if (f.n <= 32) return reg(rank_finish_reg_kernel<32>);
    if (f.n <= RANK_REG_MAX) return reg(rank_finish_reg_kernel<64>);
    if (f.n <= 128) return lds(rank_finish_lds_kernel<128>, 128);
    if (f.n <= 256) return lds(rank_finish_lds_kernel<256>, 256);
    if (f.n <= 512) return lds(rank_finish_lds_kernel<512>, 512);
    if (f.n <= 1024) return lds(rank_finish_lds_kernel<1024>, 1024);
    if (f.n <= 2048) return lds(rank_finish_lds_kernel<2048>, 2048);
    return lds(rank_finish_lds_kernel<4096>, 4096);
}

// what frog_rank_planes and frog_rank_create refuse alike without asking for a device
int rank_arguments(const char *where, const frog_volume *grid, uint32_t n_images, const void *out, size_t *total)
{
    if (int rc = group_arguments(where, grid, out, total)) return rc;
    if (!n_images || n_images > FROG_RANK_MAX_IMAGES)
        return fail(FROG_E_INVALID, std::string(where) + ": 1 to " + std::to_string(FROG_RANK_MAX_IMAGES) + " images");
    return FROG_OK;
}

// ---- the coverage-aware Gaussian (k_smooth.hip.h) of frog_smooth_volume and frog_glm_smooth ------------------------------------

// The taps of the three axes of `grid`, as frog_smooth_taps gives them; sigma == 0: radius 0 and w_0 = 1 on every axis.
int smooth_taps3(const char *where, const frog_volume *grid, double sigma, SmoothTaps taps[3])
{
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) return fail(FROG_E_INVALID, std::string(where) + ": sigma is finite and not negative");
    if (!voxel_count(grid)) return fail(FROG_E_INVALID, "empty grid");
    for (int k = 0; k < 3; k++) {
        taps[k] = SmoothTaps{};
        taps[k].w[0] = 1.0;
        if (sigma == 0.0) continue;
        if (int rc = frog_smooth_taps(sigma, grid->spacing[k], &taps[k].radius, taps[k].w)) return rc;      // with its message
    }
    return FROG_OK;
}

// the free bytes of the current device, as frog_glm_smooth and frog_glm_smooth_planes count them
// (test hook: FROG_CHAIN_FREE_MAX=n, at most n of them count; read at every call)
hipError_t smooth_free_bytes(size_t *free_bytes)
{
    size_t device_bytes = 0;
    const hipError_t e = hipMemGetInfo(free_bytes, &device_bytes);
    const char *s = getenv("FROG_CHAIN_FREE_MAX");
    const long long cap = s ? atoll(s) : 0;
    if (e == hipSuccess && cap > 0) *free_bytes = std::min(*free_bytes, (size_t)cap);
    return e;
}

hipError_t smooth_work_alloc(SmoothWork &w, size_t count)
{
    hipError_t e = w.d_raw.alloc(count);
    if (e == hipSuccess) e = w.d_x.alloc(count);
    if (e == hipSuccess) e = w.d_y.alloc(count);
    return e;
}

// The three passes over the `count` voxels in w.d_raw, whole planes of `grid` (with the flags d_take of the same voxels, or
// null); d_out receives the `window` voxels from `offset` on.
hipError_t smooth_passes(const frog_volume &grid, SmoothWork &w, const uint8_t *d_take, size_t count, size_t offset, size_t window, float *d_out)
{
    const uint32_t nx = grid.dims[0], ny = grid.dims[1];
    hipError_t e = chunked_launch(count, [&](unsigned blocks, size_t base) {
        smooth_x_kernel<<<blocks, LAUNCH_BLOCK>>>(base, count, nx, w.d_raw.p, d_take, w.taps[0], w.d_x.p);
    });
    if (e == hipSuccess) e = chunked_launch(count, [&](unsigned blocks, size_t base) {
        smooth_y_kernel<<<blocks, LAUNCH_BLOCK>>>(base, count, nx, ny, w.d_x.p, w.taps[1], w.d_y.p);
    });
    if (e == hipSuccess) e = chunked_launch(window, [&](unsigned blocks, size_t base) {
        smooth_z_kernel<<<blocks, LAUNCH_BLOCK>>>(base, window, offset, count, (size_t)nx * ny, w.d_raw.p, d_take, w.d_y.p, w.taps[2], d_out);
    });
    return e;
}

// the second half of a smoothed add: the raw map of the range is in the scratch
int glm_smooth_store(const char *where, frog_glm *a)
{
    SmoothPlan &s = a->smooth;
    hipError_t e = smooth_passes(a->grid, s.work, nullptr, s.count, a->first - s.first, a->window, a->d_vals.p + (size_t)a->added * a->window);
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) return hip_fail(where, e);
    a->added++;
    return FROG_OK;
}

// the planes [*first, *first + *count) a window's smoothed add evaluates
void smooth_range(uint32_t depth, uint32_t first_plane, uint32_t n_planes, uint32_t radius, uint32_t *first, uint32_t *count)
{
    *first = first_plane > radius ? first_plane - radius : 0;
    *count = (uint32_t)std::min<uint64_t>((uint64_t)first_plane + n_planes + radius, depth) - *first;
}

// what frog_glm_finish and frog_glm_permute refuse alike, before the device is touched
int glm_fit_arguments(const char *where, const frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor)
{
    const std::string w = std::string(where) + ": ";
    if (!a || n_contrasts > FROG_GLM_MAX_CONTRASTS || (n_contrasts && !contrasts)) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (a->added != a->n_images) return fail(FROG_E_INVALID, w + "fewer volumes added than n_images");
    if (!min_count) return fail(FROG_E_INVALID, w + "min_count must be at least 1");
    if (!(sigma_floor >= 0.0)) return fail(FROG_E_INVALID, w + "sigma_floor must not be negative");
    for (size_t e = 0; e < (size_t)n_contrasts * a->p; e++)
        if (!std::isfinite(contrasts[e])) return fail(FROG_E_INVALID, w + "a contrast entry is not finite");
    return FROG_OK;
}

// The fit kernel over the window for the n_perms permutations whose rows d_table holds: instantiated on the number of columns
// and on whether the values of a voxel stay in LDS.  With a sink's store, the kernel that also stores the bits or the levels.
template <int P, bool LDS>
hipError_t glm_fit_go(const frog_glm *a, const GlmArgs &f, const GlmStore &to, size_t bytes)
{
    // one block per tile: the work-items are the tiles padded to whole blocks, so a launch chunk never splits a tile
    return chunked_launch(f.tiles * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) {
        if (to.kind == GlmStore::BITS) glm_fit_kernel<P, LDS, GlmSink><<<blocks, LAUNCH_BLOCK, bytes>>>(base, a->d_vals.p, a->d_table.p, f, to.bits);
        else if (to.kind == GlmStore::LEVELS) glm_fit_kernel<P, LDS, GlmLevelSink><<<blocks, LAUNCH_BLOCK, bytes>>>(base, a->d_vals.p, a->d_table.p, f, to.levels);
        else glm_fit_kernel<P, LDS><<<blocks, LAUNCH_BLOCK, bytes>>>(base, a->d_vals.p, a->d_table.p, f);
    });
}

hipError_t glm_fit_launch(const frog_glm *a, const GlmArgs &f, const GlmStore &sink = GlmStore{})
{
    const bool lds = a->n_images <= GLM_LDS_MAX;
    const size_t bytes = (f.extrema ? (size_t)f.n_perms * f.n_contrasts * 2 * sizeof(uint32_t) : 0) + (lds ? (size_t)a->n_images * 256 * sizeof(float) : 0);
    switch (a->p * 2 + (lds ? 1 : 0)) {
    case 2: return glm_fit_go<1, false>(a, f, sink, bytes);
    case 3: return glm_fit_go<1, true>(a, f, sink, bytes);
    case 4: return glm_fit_go<2, false>(a, f, sink, bytes);
    case 5: return glm_fit_go<2, true>(a, f, sink, bytes);
    case 6: return glm_fit_go<3, false>(a, f, sink, bytes);
    case 7: return glm_fit_go<3, true>(a, f, sink, bytes);
    case 8: return glm_fit_go<4, false>(a, f, sink, bytes);
    case 9: return glm_fit_go<4, true>(a, f, sink, bytes);
    case 10: return glm_fit_go<5, false>(a, f, sink, bytes);
    case 11: return glm_fit_go<5, true>(a, f, sink, bytes);
    case 12: return glm_fit_go<6, false>(a, f, sink, bytes);
    case 13: return glm_fit_go<6, true>(a, f, sink, bytes);
    case 14: return glm_fit_go<7, false>(a, f, sink, bytes);
    case 15: return glm_fit_go<7, true>(a, f, sink, bytes);
    case 16: return glm_fit_go<8, false>(a, f, sink, bytes);
    default: return glm_fit_go<8, true>(a, f, sink, bytes);
    }
}

// the design rows of n_perms permutations (perm and sign on the device; both null: the design as it is) into a->d_table
hipError_t glm_table_launch(frog_glm *a, const uint32_t *d_perm, const int8_t *d_sign, uint32_t columns, uint32_t n_perms)
{
    const size_t total = (size_t)n_perms * a->n_images;
    hipError_t e = a->d_table.alloc(total * glm_row_doubles(a->p));
    if (e != hipSuccess) return e;
    return chunked_launch(total, [&](unsigned blocks, size_t base) {
        glm_table_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_design.p, d_perm, d_sign, a->n_images, a->p, columns, total, a->d_table.p);
    });
}

// the arguments of a launch that finish and permute fill alike; region (window-sized, may be null) goes to d_region
int glm_fit_args(const char *where, frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                 const uint8_t *region, frog::DevBuf<uint8_t> &d_region, GlmArgs *f)
{
    *f = GlmArgs{};
    f->window = a->window;
    f->tiles = (a->window + GLM_TILE - 1) / GLM_TILE;
    f->n = a->n_images;
    f->need = std::max(min_count, a->p + 1u);
    f->n_contrasts = n_contrasts;
    f->sigma_floor = sigma_floor;
    for (size_t e = 0; e < (size_t)n_contrasts * a->p; e++) f->contrasts[e] = contrasts[e];
    if (region) {
        KCHECK(d_region.alloc(a->window));
        const hipError_t e = hipMemcpy(d_region.p, region, a->window, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(where, e);
        f->region = d_region.p;
    }
    return FROG_OK;
}

// frog_glm_permute (no sink), frog_glm_permute_clusters and frog_glm_permute_tfce (one sink): the validation, the table batches
// and the launches, which with a sink store the bits or the levels of row k in the sink's permutation first_perm + k
int glm_permute(const char *where, frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign, uint32_t first_perm,
                frog_sink *sink, float *max_t, float *min_t)
{
    const std::string w = std::string(where) + ": ";
    if (int rc = glm_fit_arguments(where, a, n_contrasts, contrasts, min_count, sigma_floor)) return rc;
    if (!n_contrasts || !n_perms || !perm || (!sink && !max_t && !min_t)) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (!columns || (columns >> a->p)) return fail(FROG_E_INVALID, w + "columns names at least one column, and none past the design's");
    const size_t entries = (size_t)n_perms * a->n_images;
    for (size_t e = 0; e < entries; e++) {
        if (perm[e] >= a->n_images) return fail(FROG_E_INVALID, w + "a perm entry is not an image index");
        if (sign && sign[e] != 1 && sign[e] != -1) return fail(FROG_E_INVALID, w + "a sign is +1 or -1");
    }
    const size_t plane = (size_t)a->grid.dims[0] * a->grid.dims[1];
    const uint32_t z0 = (uint32_t)(a->first / plane), nz = (uint32_t)(a->window / plane), depth = a->grid.dims[2];
    if (sink) {
        if (sink->device != a->device) return fail(FROG_E_INVALID, w + "sink and accumulator on different devices");
        for (int k = 0; k < 3; k++)
            if (sink->grid.dims[k] != a->grid.dims[k]) return fail(FROG_E_INVALID, w + "the sink's grid is not the accumulator's");
        if (n_contrasts != sink->n_contrasts) return fail(FROG_E_INVALID, w + "the sink was created for another number of contrasts");
        if (first_perm > sink->n_perms || n_perms > sink->n_perms - first_perm) return fail(FROG_E_INVALID, w + "permutations beyond the sink's");
        for (uint32_t k = 0; k < n_perms; k++)
            for (uint32_t z = 0; z < nz; z++)
                if (sink->received[(size_t)(first_perm + k) * depth + z0 + z])
                    return fail(FROG_E_STATE, w + "plane " + std::to_string(z0 + z) + " of permutation " + std::to_string(first_perm + k) + " has been written before");
    }
    KCHECK(hipSetDevice(a->device));
    const size_t n_ext = (size_t)n_perms * n_contrasts * 2;
    frog::DevBuf<uint32_t> d_perm, d_ext;
    frog::DevBuf<int8_t> d_sign;
    frog::DevBuf<uint8_t> d_region;
    KCHECK(d_perm.alloc(entries));
    KCHECK(d_ext.alloc(n_ext));
    if (sign) KCHECK(d_sign.alloc(entries));
    std::vector<uint32_t> ext(n_ext);
    for (size_t e = 0; e < n_ext; e++) ext[e] = (e & 1) ? GLM_KEY_POS_INF : GLM_KEY_NEG_INF;
    GlmArgs f;
    if (int rc = glm_fit_args(where, a, n_contrasts, contrasts, min_count, sigma_floor, region, d_region, &f)) return rc;
    GlmStore to = sink ? sink->store : GlmStore{};  // what the sink wants stored, at this window
    to.bits.first = to.levels.first = a->first;
    hipError_t e = hipMemcpy(d_perm.p, perm, entries * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && sign) e = hipMemcpy(d_sign.p, sign, entries, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_ext.p, ext.data(), n_ext * sizeof(uint32_t), hipMemcpyHostToDevice);
    // the permutations in launches of at most GLM_BATCH whose design rows fit GLM_TABLE_BYTES
    const size_t per_perm = (size_t)a->n_images * glm_row_doubles(a->p) * sizeof(double);
    const uint32_t batch = (uint32_t)std::max<size_t>(1, std::min<size_t>(GLM_BATCH, GLM_TABLE_BYTES / per_perm));
    for (uint32_t k0 = 0; k0 < n_perms && e == hipSuccess; k0 += batch) {
        const uint32_t nb = std::min(batch, n_perms - k0);
        const size_t at = (size_t)k0 * a->n_images;
        e = glm_table_launch(a, d_perm.p + at, sign ? d_sign.p + at : nullptr, columns, nb);
        f.n_perms = nb;
        f.extrema = d_ext.p + (size_t)k0 * n_contrasts * 2;
        to.bits.perm0 = to.levels.perm0 = first_perm + k0;
        if (e == hipSuccess) e = glm_fit_launch(a, f, to);
    }
    if (e == hipSuccess) e = hipMemcpy(ext.data(), d_ext.p, n_ext * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(where, e);
    for (uint32_t k = 0; sink && k < n_perms; k++) std::fill_n(sink->received.begin() + (size_t)(first_perm + k) * depth + z0, nz, (uint8_t)1);
    for (size_t e2 = 0; e2 < n_ext / 2; e2++) {
        const uint32_t hi = ext[2 * e2], lo = ext[2 * e2 + 1];
        const uint32_t bits_hi = (hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi, bits_lo = (lo & 0x80000000u) ? (lo ^ 0x80000000u) : ~lo;
        if (max_t) std::memcpy(max_t + e2, &bits_hi, sizeof(float));
        if (min_t) std::memcpy(min_t + e2, &bits_lo, sizeof(float));
    }
    return FROG_OK;
}

// ---- connected components (k_ccl.hip.h) ---------------------------------------------------------------------------------------

// the largest |dx| + |dy| + |dz| of a neighbour at connectivity 6, 18 or 26; 0 for anything else
uint32_t ccl_order(int connectivity) { return connectivity == 6 ? 1u : connectivity == 18 ? 2u : connectivity == 26 ? 3u : 0u; }

CclGrid ccl_grid(const frog_volume *grid, size_t total, int connectivity)
{
    return CclGrid{ grid->dims[0], grid->dims[1], grid->dims[2], ccl_order(connectivity), (total + 31) / 32, total };
}

// The components of n_masks <= the workspace's masks, `words` apart from d_masks on: parents and extents at the set voxels of
// the workspace, and with d_stats (2 words per mask, zero) the components' number and the largest extent.
hipError_t ccl_label(const CclGrid &g, const uint32_t *d_masks, uint32_t n_masks, uint32_t *d_parent, uint32_t *d_extent, uint32_t *d_stats)
{
    hipError_t e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
        ccl_init_kernel<<<dim3(blocks, n_masks), LAUNCH_BLOCK>>>(base, d_masks, g, d_parent, d_extent);
    });
    if (e == hipSuccess) e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
        ccl_link_kernel<<<dim3(blocks, n_masks), LAUNCH_BLOCK>>>(base, d_masks, g, d_parent);
    });
    if (e == hipSuccess) e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
        ccl_count_kernel<<<dim3(blocks, n_masks), LAUNCH_BLOCK>>>(base, d_masks, g, d_parent, d_extent);
    });
    if (e == hipSuccess && d_stats) e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
        ccl_stats_kernel<<<dim3(blocks, n_masks), LAUNCH_BLOCK>>>(base, d_masks, g, d_parent, d_extent, d_stats);
    });
    return e;
}

// One labelled mask as labels 1..K in ascending order of root, into the host array: the device writes root + 1, and since a
// root is the smallest index of its component, one ascending host pass numbers a root when it meets it and copies the
// number to the members that follow.  Returns K through n.
hipError_t ccl_labels_out(const CclGrid &g, const uint32_t *d_mask, const uint32_t *d_parent, uint32_t *labels, uint32_t *n)
{
    frog::DevBuf<uint32_t> d_out;
    hipError_t e = d_out.alloc(g.total);
    if (e == hipSuccess) e = chunked_launch(g.total, [&](unsigned blocks, size_t base) {
        ccl_roots_kernel<<<blocks, LAUNCH_BLOCK>>>(base, d_mask, g.total, d_parent, d_out.p);
    });
    if (e == hipSuccess) e = hipMemcpy(labels, d_out.p, g.total * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    uint32_t k = 0;
    for (size_t v = 0; v < g.total; v++) {
        if (!labels[v]) continue;
        const size_t root = labels[v] - 1;
        labels[v] = root == v ? ++k : labels[root];
    }
    *n = k;
    return hipSuccess;
}

// whether every z-plane of permutations [first, first + count) has been written
bool sink_complete(const frog_sink *s, uint32_t first, uint32_t count)
{
    const size_t depth = s->grid.dims[2];
    return std::find(s->received.begin() + first * depth, s->received.begin() + ((size_t)first + count) * depth, (uint8_t)0)
           == s->received.begin() + ((size_t)first + count) * depth;
}

// how a slot's read-out begins: the refusals (with `complete`, also of a permutation that lacks planes), the slot's index, the device
int sink_slot(const char *where, const frog_sink *s, uint32_t perm, uint32_t contrast, int side, const void *out, bool complete, size_t *slot)
{
    if (!s || !out) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (perm >= s->n_perms || contrast >= s->n_contrasts || side < 0 || (uint32_t)side >= s->sides)
        return fail(FROG_E_INVALID, std::string(where) + ": no such permutation, contrast or side in the sink");
    if (complete && !sink_complete(s, perm, 1)) return fail(FROG_E_STATE, std::string(where) + ": the permutation has not received every plane of the grid");
    *slot = ((size_t)perm * s->n_contrasts + contrast) * s->sides + (uint32_t)side;
    KCHECK(hipSetDevice(s->device));
    return FROG_OK;
}

// The frame of frog_clusters_create and frog_tfce_create: the refusals, the sink's own() after the shared ones; the new sink
// with frog_sink's fields; the memory budget from sizes(ccl) = (device bytes a slot keeps, bytes of one slot's workspace), which
// holds `batch` slots: as many as fit half of what the slots leave free.  Bytes beyond size_t are refused like bytes beyond the device.
template <class S, class Own, class Sizes>
int sink_new(const char *where, const char *noun, const frog_volume *grid, uint32_t n_perms, uint32_t n_contrasts, int two_sided, int connectivity,
             int device, S **out, Own own, Sizes sizes, std::unique_ptr<S> &s)
{
    const std::string w = std::string(where) + ": ";
    size_t total, free_bytes = 0, device_bytes = 0;
    if (int rc = group_arguments(where, grid, out, &total)) return rc;
    if (!n_perms || !n_contrasts) return fail(FROG_E_INVALID, w + "at least one permutation and one contrast");
    if (n_contrasts > FROG_GLM_MAX_CONTRASTS) return fail(FROG_E_INVALID, w + "at most " + std::to_string(FROG_GLM_MAX_CONTRASTS) + " contrasts");
    if (int rc = own()) return rc;
    if (!ccl_order(connectivity)) return fail(FROG_E_INVALID, w + "connectivity 6, 18 or 26");
    if (int rc = group_new(grid, total, device, s)) return rc;
    s->n_perms = n_perms;
    s->n_contrasts = n_contrasts;
    s->sides = two_sided ? 2u : 1u;
    s->ccl = ccl_grid(grid, total, connectivity);
    s->slots = (size_t)n_perms * n_contrasts * s->sides;
    KCHECK(hipMemGetInfo(&free_bytes, &device_bytes));
    const auto [per_slot, work_bytes] = sizes(s->ccl);
    const bool countable = s->slots <= (std::numeric_limits<size_t>::max() - work_bytes) / per_slot;
    const size_t slot_bytes = countable ? s->slots * per_slot : 0;
    if (!countable || slot_bytes + work_bytes > free_bytes)
        return fail(FROG_E_NOMEM, w + std::to_string(s->slots) + " " + noun + " and the workspace need " +
                                  (countable ? std::to_string(slot_bytes + work_bytes) : std::string("more than 2^64")) + " bytes of device memory, " +
                                  std::to_string(free_bytes) + " are free");
    s->batch = (uint32_t)std::min<size_t>(std::min<size_t>(s->slots, CCL_BATCH), std::max<size_t>(1, (free_bytes - slot_bytes) / 2 / work_bytes));
    s->received.assign((size_t)n_perms * grid->dims[2], 0);
    return FROG_OK;
}

// The frame of frog_clusters_finish and frog_tfce_finish: every permutation must be complete; then each(at, n) for the slots
// [at, at + n) of every batch, and copy_out() once.
template <class Each, class Out>
int sink_finish(const char *where, frog_sink *s, const void *out, Each each, Out copy_out)
{
    if (!s || !out) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (!sink_complete(s, 0, s->n_perms)) return fail(FROG_E_STATE, std::string(where) + ": a permutation has not received every plane of the grid");
    KCHECK(hipSetDevice(s->device));
    hipError_t e = hipSuccess;
    for (size_t at = 0; at < s->slots && e == hipSuccess; at += s->batch) e = each(at, (uint32_t)std::min<size_t>(s->batch, s->slots - at));
    if (e == hipSuccess) e = copy_out();
    if (e != hipSuccess) return hip_fail(where, e);
    return FROG_OK;
}

// ---- threshold-free cluster enhancement (k_tfce.hip.h) ---------------------------------------------------------------------------

// what frog_tfce_create and frog_tfce_volume refuse alike, and the level weights w_k as the header states them
int tfce_params(const char *where, float dh, double E, double H, int connectivity, TfceParams *par)
{
    const std::string w = std::string(where) + ": ";
    if (!(dh > 0.0f) || !std::isfinite(dh)) return fail(FROG_E_INVALID, w + "dh must be finite and above 0");
    if (E != 0.5 && E != 1.0) return fail(FROG_E_INVALID, w + "E is 0.5 or 1");
    if (H != 1.0 && H != 2.0) return fail(FROG_E_INVALID, w + "H is 1 or 2");
    if (!ccl_order(connectivity)) return fail(FROG_E_INVALID, w + "connectivity 6, 18 or 26");
    par->dh = dh;
    par->root = E == 0.5;
    for (int k = 1; k <= 255; k++) {
        const double h = (double)k * (double)dh;
        const double hh = H == 2.0 ? h * h : h;
        par->weight[k] = hh * (double)dh;
    }
    return FROG_OK;
}

size_t tfce_stride(const CclGrid &g) { return g.words * 32; }

// device bytes of one slot's workspace: parent, extent, the f64 sum, the bit mask
size_t tfce_work_bytes(const CclGrid &g) { return g.total * (2 * sizeof(uint32_t) + sizeof(double)) + g.words * sizeof(uint32_t); }

hipError_t tfce_work_alloc(TfceWork &work, const CclGrid &g, size_t n)
{
    hipError_t e = work.d_bits.alloc(n * g.words);
    if (e == hipSuccess) e = work.d_parent.alloc(n * g.total);
    if (e == hipSuccess) e = work.d_extent.alloc(n * g.total);
    if (e == hipSuccess) e = work.d_acc.alloc(n * g.total);
    return e;
}

// The enhancement of the n slots whose levels lie `stride` apart from d_levels on, n at most the workspace's slots: d_top[slot]
// their highest levels, d_best[slot] the bits of their largest tfce, and with d_map (n == 1) the map.  The one device routine
// of frog_tfce_finish, frog_tfce_map and frog_tfce_volume.
hipError_t tfce_enhance(const CclGrid &g, const TfceParams &par, const uint8_t *d_levels, size_t stride, uint32_t n, TfceWork &work,
                        uint32_t *d_top, float *d_map, uint32_t *d_best)
{
    std::vector<uint32_t> top(n);
    hipError_t e = hipMemset(d_top, 0, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_best, 0, n * sizeof(uint32_t));
    if (e == hipSuccess) e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
        tfce_top_kernel<<<dim3(blocks, n), LAUNCH_BLOCK>>>(base, d_levels, stride, g.words, d_top);
    });
    if (e == hipSuccess) e = hipMemcpy(top.data(), d_top, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemset(work.d_acc.p, 0, (size_t)n * g.total * sizeof(double));
    const uint32_t highest = e == hipSuccess ? *std::max_element(top.begin(), top.end()) : 0u;
    for (uint32_t k = highest; k >= 1 && e == hipSuccess; k--) {
        e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
            tfce_mask_kernel<<<dim3(blocks, n), LAUNCH_BLOCK>>>(base, d_levels, stride, g.words, d_top, k, work.d_bits.p);
        });
        if (e == hipSuccess) e = ccl_label(g, work.d_bits.p, n, work.d_parent.p, work.d_extent.p, nullptr);
        if (e == hipSuccess) e = chunked_launch(g.words, [&](unsigned blocks, size_t base) {
            if (par.root)
                tfce_accumulate_kernel<true><<<dim3(blocks, n), LAUNCH_BLOCK>>>(base, work.d_bits.p, g, work.d_parent.p, work.d_extent.p, par.weight[k], work.d_acc.p);
            else
                tfce_accumulate_kernel<false><<<dim3(blocks, n), LAUNCH_BLOCK>>>(base, work.d_bits.p, g, work.d_parent.p, work.d_extent.p, par.weight[k], work.d_acc.p);
        });
    }
    if (e == hipSuccess) e = chunked_launch(g.total, [&](unsigned blocks, size_t base) {
        tfce_round_kernel<<<dim3(blocks, n), LAUNCH_BLOCK>>>(base, work.d_acc.p, g.total, d_map, d_best);
    });
    return e;
}

template <class S>
void ccl_pack(const S *voxels, size_t total, std::vector<uint32_t> &words)
{
    for (size_t v = 0; v < total; v++)
        if (voxels[v] != 0) words[v >> 5] |= 1u << (v & 31);
}

// frog_staple_add for a source of type S: labels_add_typed with the index plane in place of the vote.  The plane of the
// image is written, and its labels become known, only after the volume's labels are accepted and its plane is complete, so a
// refused volume leaves nothing behind.
template <class S>
int staple_add_typed(frog_staple *a, frog_chain *c, const frog_volume *src, double background, frog_volume *resliced)
{
    const S *d_labels;
    size_t n_now;
    if (int rc = labels_collect<S>("frog_staple_add", a, a, c, src, background, &d_labels, &n_now)) return rc;
    std::vector<long long> fresh;
    hipError_t e = labels_fresh_values(a, n_now, fresh);
    if (e != hipSuccess) return labels_refuse(a, hip_fail("frog_staple_add", e));
    uint8_t *plane = a->d_D.p + (size_t)a->added * a->total;
    e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        staple_index_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, d_labels, a->total, a->map, plane);
    });
    const int rc = return_resliced<S>("frog_staple_add", a, c, src, resliced, e);
    if (rc != FROG_OK) return labels_refuse(a, rc);
    a->known.insert(a->known.end(), fresh.begin(), fresh.end());
    return FROG_OK;
}

// one E-step over the grid: the smallest register tile that holds the labels, the largest tiled above it
hipError_t staple_estep_launch(const frog_staple *a)
{
    const uint32_t L = (uint32_t)a->values.size();
    auto run = [&](auto kernel) {
        return chunked_launch(a->total, [&](unsigned blocks, size_t base) {
            kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_D.p, a->total, a->n_images, L, a->d_theta.p, a->d_prior.p, a->d_active.p, a->d_q.p);
        });
    };
    if (L <= 4) return run(staple_estep_kernel<4>);
    if (L <= 8) return run(staple_estep_kernel<8>);
    if (L <= 16) return run(staple_estep_kernel<16>);
    return run(staple_estep_kernel<(int)STAPLE_TILE_MAX>);
}

// STAPLE_MSTEP_UNIFORM=0 at build time: every wave of the M-step takes the per-lane path (the A/B of DESIGN 20)
#ifndef STAPLE_MSTEP_UNIFORM
#define STAPLE_MSTEP_UNIFORM 1
#endif

// one M-step: S zeroed and summed, T, then theta and *change
int staple_mstep(frog_staple *a, double *change)
{
    const uint32_t L = (uint32_t)a->values.size();
    const size_t entries = (size_t)a->n_images * L * L;
    unsigned long long *d_change = a->d_word.p + L;
    const StapleTiles t = staple_tiles(a->n_images, L, a->total);
    KCHECK(hipMemset(a->d_S.p, 0, entries * sizeof(unsigned long long)));
    KCHECK(hipMemset(d_change, 0, sizeof(unsigned long long)));
    KCHECK(chunked_launch((size_t)t.tiles * t.per_tile * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) {
        staple_mstep_kernel<STAPLE_MSTEP_UNIFORM != 0><<<blocks, LAUNCH_BLOCK>>>(base, a->d_D.p, a->total, t, a->d_active.p, a->d_q.p, a->d_S.p);
    }));
    KCHECK(chunked_launch(L, [&](unsigned blocks, size_t base) {
        staple_totals_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_S.p, L, a->d_T.p);
    }));
    KCHECK(chunked_launch(entries, [&](unsigned blocks, size_t base) {
        staple_theta_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_S.p, a->d_T.p, L, entries, a->d_theta.p, d_change);
    }));
    unsigned long long bits = 0;
    KCHECK(hipMemcpy(&bits, d_change, sizeof bits, hipMemcpyDeviceToHost));
    std::memcpy(change, &bits, sizeof bits);
    return FROG_OK;
}

// ---- the distance transform and the surface distances (k_edt.hip.h) ----------------------------------------------------------

bool edt_spacing(const frog_volume *v)
{
    for (int k = 0; k < 3; k++)
        if (!(v->spacing[k] > 0.0) || !std::isfinite(v->spacing[k])) return false;
    return true;
}

// the box lo .. hi (inclusive) of the grid
EdtBox edt_box(const frog_volume &grid, const uint32_t lo[3], const uint32_t hi[3])
{
    EdtBox b;
    b.x0 = lo[0]; b.y0 = lo[1]; b.z0 = lo[2];
    b.nx = hi[0] - lo[0] + 1; b.ny = hi[1] - lo[1] + 1; b.nz = hi[2] - lo[2] + 1;
    b.gx = grid.dims[0]; b.gy = grid.dims[1];
    b.sx = grid.spacing[0]; b.sy = grid.spacing[1]; b.sz = grid.spacing[2];
    return b;
}

EdtBox edt_whole(const frog_volume &grid)
{
    const uint32_t lo[3] = { 0, 0, 0 }, hi[3] = { grid.dims[0] - 1, grid.dims[1] - 1, grid.dims[2] - 1 };
    return edt_box(grid, lo, hi);
}

size_t edt_box_voxels(const EdtBox &b) { return (size_t)b.nx * b.ny * b.nz; }

// The x and y passes over box b for the features idx == l (surface_only: and surf): g2 holds the result, `any` the planes with
// a feature.  g1 and g2 grow to the box; `any` holds the grid's planes + 1 words.
hipError_t edt_xy(const EdtBox &b, const uint16_t *idx, const uint8_t *surf, uint32_t l, int surface_only, frog::DevBuf<double> &g1,
                  frog::DevBuf<double> &g2, uint32_t *any)
{
    const size_t count = edt_box_voxels(b), lines = (size_t)b.ny * b.nz;
    hipError_t e = g1.alloc(count);
    if (e == hipSuccess) e = g2.alloc(count);
    if (e == hipSuccess) e = hipMemsetAsync(any, 0, ((size_t)b.nz + 1) * sizeof(uint32_t), 0);
    if (e == hipSuccess) e = chunked_launch(lines * 64, [&](unsigned blocks, size_t base) {
        edt_x_kernel<<<blocks, LAUNCH_BLOCK>>>(base, b, idx, surf, l, surface_only, g1.p, any);
    });
    if (e == hipSuccess) e = chunked_launch(count, [&](unsigned blocks, size_t base) {
        edt_y_kernel<<<blocks, LAUNCH_BLOCK>>>(base, b, g1.p, g2.p, any);
    });
    return e;
}

// The transform over box b as stored distances, out indexed by the box.
hipError_t edt_map(const EdtBox &b, const uint16_t *idx, const uint8_t *surf, uint32_t l, int surface_only, frog::DevBuf<double> &g1,
                   frog::DevBuf<double> &g2, uint32_t *any, uint32_t *out)
{
    hipError_t e = edt_xy(b, idx, surf, l, surface_only, g1, g2, any);
    if (e == hipSuccess) e = chunked_launch(edt_box_voxels(b), [&](unsigned blocks, size_t base) {
        edt_z_kernel<<<blocks, LAUNCH_BLOCK>>>(base, b, g2.p, any, out);
    });
    return e;
}

// idx and surf of a label volume of S on the grid (device pointers)
template <class S>
hipError_t edt_surface(const frog_volume &grid, size_t total, const S *d_labels, const long long *d_values, uint32_t n, uint16_t *idx, uint8_t *surf)
{
    return chunked_launch(total, [&](unsigned blocks, size_t base) {
        edt_surface_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, d_labels, grid.dims[0], grid.dims[1], grid.dims[2], d_values, n, idx, surf);
    });
}

// per value the box of its set and the number of its surface voxels, to the host
hipError_t edt_bounds(const frog_volume &grid, size_t total, const uint16_t *idx, const uint8_t *surf, uint32_t n, uint32_t *d_bounds,
                      std::vector<uint32_t> &bounds)
{
    bounds.assign((size_t)n * EDT_BOUND_WORDS, 0u);
    for (uint32_t l = 0; l < n; l++)
        for (int k = 0; k < 3; k++) bounds[(size_t)l * EDT_BOUND_WORDS + k] = 0xFFFFFFFFu;
    hipError_t e = hipMemcpy(d_bounds, bounds.data(), bounds.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = chunked_launch(total, [&](unsigned blocks, size_t base) {
        edt_bounds_kernel<<<blocks, LAUNCH_BLOCK>>>(base, idx, surf, grid.dims[0], grid.dims[1], total, d_bounds);
    });
    if (e == hipSuccess) e = hipMemcpy(bounds.data(), d_bounds, bounds.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return e;
}

template <class S>
int distance_map_typed(const frog_volume *labels, size_t total, long long value, int mode, uint32_t *out)
{
    frog::DevBuf<S> d_labels;
    frog::DevBuf<long long> d_value;
    frog::DevBuf<uint16_t> d_idx;
    frog::DevBuf<uint8_t> d_surf;
    frog::DevBuf<double> g1, g2;
    frog::DevBuf<uint32_t> d_any, d_out;
    KCHECK(d_labels.alloc(total));
    KCHECK(d_value.alloc(1));
    KCHECK(d_idx.alloc(total));
    KCHECK(d_surf.alloc(total));
    KCHECK(d_any.alloc((size_t)labels->dims[2] + 1));
    KCHECK(d_out.alloc(total));
    hipError_t e = hipMemcpy(d_labels.p, labels->data, total * sizeof(S), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_value.p, &value, sizeof value, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = edt_surface<S>(*labels, total, d_labels.p, d_value.p, 1, d_idx.p, d_surf.p);
    if (e == hipSuccess) e = edt_map(edt_whole(*labels), d_idx.p, d_surf.p, 0, mode, g1, g2, d_any.p, d_out.p);
    if (e == hipSuccess) e = hipMemcpy(out, d_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_distance_map", e);
    return FROG_OK;
}

// frog_surface_create for a reference of type S: idx, surf, the boxes and one whole-grid map per value
template <class S>
int surface_create_typed(frog_surface *a, const frog_volume *reference)
{
    const uint32_t n = (uint32_t)a->values.size();
    KCHECK(a->d_src.alloc(a->total * sizeof(S)));
    KCHECK(a->d_values.alloc(n));
    KCHECK(a->d_ref_idx.alloc(a->total));
    KCHECK(a->d_ref_surf.alloc(a->total));
    KCHECK(a->d_idx.alloc(a->total));
    KCHECK(a->d_surf.alloc(a->total));
    KCHECK(a->d_maps.alloc((size_t)n * a->total));
    KCHECK(a->d_bounds.alloc((size_t)n * EDT_BOUND_WORDS));
    KCHECK(a->d_any.alloc((size_t)a->grid.dims[2] + 1));
    KCHECK(a->d_largest.alloc(2 * (size_t)n));
    KCHECK(a->d_sum.alloc(2 * (size_t)n));
    KCHECK(a->d_count.alloc(1));
    hipError_t e = hipMemcpy(a->d_src.p, reference->data, a->total * sizeof(S), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a->d_values.p, a->values.data(), n * sizeof(long long), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = edt_surface<S>(a->grid, a->total, (const S *)a->d_src.p, a->d_values.p, n, a->d_ref_idx.p, a->d_ref_surf.p);
    if (e == hipSuccess) e = edt_bounds(a->grid, a->total, a->d_ref_idx.p, a->d_ref_surf.p, n, a->d_bounds.p, a->ref_bounds);
    const EdtBox whole = edt_whole(a->grid);
    for (uint32_t l = 0; l < n && e == hipSuccess; l++) {
        uint32_t *map = a->d_maps.p + (size_t)l * a->total;
        if (!a->ref_bounds[(size_t)l * EDT_BOUND_WORDS + 6]) e = hipMemsetAsync(map, 0xFF, a->total * sizeof(uint32_t), 0);
        else e = edt_map(whole, a->d_ref_idx.p, a->d_ref_surf.p, l, 1, a->d_g1, a->d_g2, a->d_any.p, map);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) return hip_fail("frog_surface_create", e);
    return FROG_OK;
}

// the k-th smallest (1-based) of a non-empty list
uint32_t edt_kth(std::vector<uint32_t> &d, uint64_t k)
{
    std::nth_element(d.begin(), d.begin() + (k - 1), d.end());
    return d[k - 1];
}

// frog_surface_add for a source of type S
template <class S>
int surface_add_typed(frog_surface *a, frog_chain *c, const frog_volume *src, double background, frog_surface_row *rows)
{
    const char *where = "frog_surface_add";
    ResliceGrid g;
    if (int rc = stage_source<S>(where, a, src, c != nullptr, 0, background, &g)) return rc;
    const S *d_src = (const S *)a->d_src.p;
    S *d_out = (S *)a->d_out.p;
    const S *d_labels = c ? d_out : d_src;
    const uint32_t n = (uint32_t)a->values.size();
    hipError_t e = hipSuccess;
    if (c) e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        reslice_kernel<S><<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_src, g, d_out);
    });
    if (e == hipSuccess) e = edt_surface<S>(a->grid, a->total, d_labels, a->d_values.p, n, a->d_idx.p, a->d_surf.p);
    std::vector<uint32_t> bounds;
    if (e == hipSuccess) e = edt_bounds(a->grid, a->total, a->d_idx.p, a->d_surf.p, n, a->d_bounds.p, bounds);
    if (e != hipSuccess) return hip_fail(where, e);
    auto n_a = [&](uint32_t l) { return (uint64_t)bounds[(size_t)l * EDT_BOUND_WORDS + 6]; };
    auto n_b = [&](uint32_t l) { return (uint64_t)a->ref_bounds[(size_t)l * EDT_BOUND_WORDS + 6]; };
    size_t capacity = 0;
    for (uint32_t l = 0; l < n; l++) capacity += n_a(l) + (n_a(l) ? n_b(l) : 0);
    KCHECK(a->d_list.alloc(capacity));
    const EdtList list{ a->d_list.p, a->d_count.p };
    e = hipMemsetAsync(a->d_sum.p, 0, 2 * (size_t)n * sizeof(unsigned long long), 0);
    if (e == hipSuccess) e = hipMemsetAsync(a->d_largest.p, 0, 2 * (size_t)n * sizeof(uint32_t), 0);
    if (e == hipSuccess) e = hipMemsetAsync(a->d_count.p, 0, sizeof(unsigned long long), 0);
    if (e == hipSuccess) e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        edt_read_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_idx.p, a->d_surf.p, a->total, a->d_maps.p, a->d_sum.p, a->d_largest.p, list);
    });
    for (uint32_t l = 0; l < n && e == hipSuccess; l++) {
        if (!n_a(l) || !n_b(l)) continue;
        const uint32_t *pa = &bounds[(size_t)l * EDT_BOUND_WORDS], *pb = &a->ref_bounds[(size_t)l * EDT_BOUND_WORDS];
        uint32_t lo[3], hi[3];
        for (int k = 0; k < 3; k++) { lo[k] = std::min(pa[k], pb[k]); hi[k] = std::max(pa[3 + k], pb[3 + k]); }
        const EdtBox b = edt_box(a->grid, lo, hi);
        e = edt_xy(b, a->d_idx.p, a->d_surf.p, l, 1, a->d_g1, a->d_g2, a->d_any.p);
        if (e == hipSuccess) e = chunked_launch(edt_box_voxels(b), [&](unsigned blocks, size_t base) {
            edt_z_collect_kernel<<<blocks, LAUNCH_BLOCK>>>(base, b, a->d_g2.p, a->d_ref_idx.p, a->d_ref_surf.p, l, n + l, a->d_sum.p + n,
                                                          a->d_largest.p + n, list);
        });
    }
    std::vector<unsigned long long> sum(2 * (size_t)n);
    std::vector<uint32_t> largest(2 * (size_t)n);
    unsigned long long count = 0;
    if (e == hipSuccess) e = hipMemcpy(sum.data(), a->d_sum.p, sum.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(largest.data(), a->d_largest.p, largest.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&count, a->d_count.p, sizeof count, hipMemcpyDeviceToHost);
    if (e == hipSuccess && count != capacity) return fail(FROG_E_HIP, std::string(where) + ": the distance list is incomplete");
    std::vector<uint2> entries(capacity);
    if (e == hipSuccess && capacity) e = hipMemcpy(entries.data(), a->d_list.p, capacity * sizeof(uint2), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(where, e);
    // the percentile: an order statistic of each key's distances, whatever order the list has them in
    std::vector<std::vector<uint32_t>> by_key(2 * (size_t)n);
    for (uint32_t l = 0; l < n; l++) {
        if (!n_a(l) || !n_b(l)) continue;
        by_key[l].reserve(n_a(l));
        by_key[n + l].reserve(n_b(l));
    }
    for (const uint2 &x : entries)
        if (n_b(x.x % n)) by_key[x.x].push_back(x.y);
    for (uint32_t l = 0; l < n; l++) {
        frog_surface_row &r = rows[l];
        r.n_a = n_a(l); r.n_b = n_b(l);
        r.sum_ab = r.sum_ba = 0;
        r.max_ab = r.max_ba = r.pct_ab = r.pct_ba = 0xFFFFFFFFu;
        if (!r.n_a || !r.n_b) continue;
        if (by_key[l].size() != r.n_a || by_key[n + l].size() != r.n_b) return fail(FROG_E_HIP, std::string(where) + ": the distance list is incomplete");
        r.sum_ab = sum[l]; r.sum_ba = sum[n + l];
        r.max_ab = largest[l]; r.max_ba = largest[n + l];
        r.pct_ab = edt_kth(by_key[l], ((uint64_t)a->percentile * r.n_a + 99) / 100);
        r.pct_ba = edt_kth(by_key[n + l], ((uint64_t)a->percentile * r.n_b + 99) / 100);
    }
    return FROG_OK;
}

// What frog_glm_add_jacobian and frog_modes' chain adds refuse alike, before the device is touched; a good mask is left in
// a->h_mask.
int chain_add_inputs(const char *where, frog_windowed *a, const frog_chain *c, const frog_volume *support, const frog_volume *mask)
{
    const std::string w = std::string(where) + ": ";
    if (!a || !c) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (a->added >= a->n_images) return fail(FROG_E_INVALID, w + "more volumes than the accumulator was created for");
    if (c->device != a->device) return fail(FROG_E_INVALID, w + "chain and accumulator on different devices");
    if (support && (!voxel_count(support) || !chain_samples(support))) return fail(FROG_E_INVALID, w + "bad support geometry");
    if (mask) {
        if (!mask->data) return fail(FROG_E_INVALID, w + "a mask without voxels");
        if (!integer_voxel_type(mask->dtype)) return fail(FROG_E_INVALID, w + "a mask has an integer type");
        if (!voxel_count(mask) || !chain_samples(mask)) return fail(FROG_E_INVALID, w + "bad mask geometry");
        cover_mask(a, mask);
    }
    return FROG_OK;
}

// glm_jacobian_kernel over the `window` voxels of the grid from `first` on, into `plane`; the add is not counted
int jacobian_launch(const char *where, frog_windowed *a, frog_chain *c, const frog_volume *support, const frog_volume *mask, int log_mode,
                    size_t first, size_t window, float *plane)
{
    KCHECK(hipSetDevice(a->device));
    const uint8_t *d_mask;
    if (int rc = cover_stage_mask(where, a, mask, &d_mask)) return rc;
    const MaskGrid mg = mask_grid(mask), sg = mask_grid(support);
    const NodeGrid out = node_grid(a->grid.origin, a->grid.spacing, a->grid.dims);
    const hipError_t e = chunked_launch(window, [&](unsigned blocks, size_t base) {
        glm_jacobian_kernel<<<blocks, LAUNCH_BLOCK>>>(base, first, window, c->d_links.p, (int)c->h_links.size(), out, support != nullptr, sg,
                                                      d_mask, mg, log_mode != 0, plane);
    });
    if (e != hipSuccess) return hip_fail(where, e);
    return FROG_OK;
}

// the end of an add that launched on the null stream: wait, then count it
int windowed_added(const char *where, frog_windowed *a)
{
    const hipError_t e = hipStreamSynchronize(0);
    if (e != hipSuccess) return hip_fail(where, e);
    a->added++;
    return FROG_OK;
}

// ---- the principal modes of a group (k_modes.hip.h) ---------------------------------------------------------------------------

constexpr size_t MODES_SCRATCH_BYTES = (size_t)256 << 20;      // what a batch of gram or project may take, beyond one plane's
constexpr size_t MODES_BATCH_CHUNKS = (size_t)1 << 20;         // the most chunks of one launch: well inside a dispatch's 32-bit grid

// what frog_modes_planes and frog_modes_create refuse alike without asking for a device
int modes_arguments(const char *where, const frog_volume *grid, uint32_t n_images, uint32_t n_components, const void *out, size_t *total)
{
    if (int rc = group_arguments(where, grid, out, total)) return rc;
    if (n_images < 2 || n_images > FROG_MODES_MAX_IMAGES)
        return fail(FROG_E_INVALID, std::string(where) + ": 2 to " + std::to_string(FROG_MODES_MAX_IMAGES) + " images");
    if (n_components != 1 && n_components != 3) return fail(FROG_E_INVALID, std::string(where) + ": 1 or 3 components");
    return FROG_OK;
}

// what gram and project refuse alike; region (window-sized, may be null) goes to d_region
int modes_ready(const char *where, const frog_modes *a)
{
    if (a->added != a->n_images) return fail(FROG_E_INVALID, std::string(where) + ": fewer volumes added than n_images");
    return FROG_OK;
}

int modes_region(const char *where, const frog_modes *a, const uint8_t *region, frog::DevBuf<uint8_t> &d_region)
{
    if (!region) return FROG_OK;
    KCHECK(d_region.alloc(a->window));
    const hipError_t e = hipMemcpy(d_region.p, region, a->window, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(where, e);
    return FROG_OK;
}

// the chain on n f32 points that lie on the chain's device (in and out may be the same array)
hipError_t chain_apply_f32_device(frog_chain *c, const float *d_in, float *d_out, size_t n)
{
    return chunked_launch(n, [&](unsigned blocks, size_t base) {
        chain_apply_f32_kernel<<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_in, d_out, n);
    });
}

// frog_isosurface_create refuses a result of ISO_RESULT_MAX or more vertices or triangles: the indices are 32-bit and a mesh
// file's counts signed
// (test hook: FROG_ISO_RESULT_MAX=n lowers the limit)
uint64_t iso_result_max()
{
    static const uint64_t m = [] {
        const uint64_t cap = (uint64_t)1 << 31;
        const char *s = getenv("FROG_ISO_RESULT_MAX");
        const long long v = s ? atoll(s) : 0;
        return v > 0 ? std::min(cap, (uint64_t)v) : cap;
    }();
    return m;
}

// exclusive sums of the blocks' totals: d_sums[b] for block b, d_sums[blocks] the grand total (d_counts has blocks + 1 entries,
// the last one zero)
int iso_block_offsets(const frog::DevBuf<unsigned long long> &d_counts, frog::DevBuf<unsigned long long> &d_sums, size_t blocks,
                      frog::DevBuf<unsigned char> &d_temp, uint64_t *grand)
{
    size_t bytes = 0;
    KCHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_counts.p, d_sums.p, blocks + 1));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceScan::ExclusiveSum(d_temp.p, bytes, d_counts.p, d_sums.p, blocks + 1));
    unsigned long long total = 0;
    KCHECK(hipMemcpy(&total, d_sums.p + blocks, sizeof total, hipMemcpyDeviceToHost));
    *grand = total;
    return FROG_OK;
}

template <class S>
int isosurface_typed(frog_isosurface *s, const frog_volume *v, size_t total, int mode, double level, long long value)
{
    IsoParams p;
    p.g = node_grid(v->origin, v->spacing, v->dims);
    p.mode = mode; p.level = level; p.value = value;
    const size_t blocks = (total + ISO_BLOCK - 1) / ISO_BLOCK;
    frog::DevBuf<S> d_vol;
    frog::DevBuf<uint8_t> d_mask, d_config;
    frog::DevBuf<unsigned long long> d_count_v, d_count_t, d_first_v, d_first_t;
    frog::DevBuf<unsigned char> d_temp;
    KCHECK(d_vol.alloc(total));
    KCHECK(d_mask.alloc(total));
    KCHECK(d_config.alloc(total));
    KCHECK(d_count_v.alloc(blocks + 1));
    KCHECK(d_count_t.alloc(blocks + 1));
    KCHECK(d_first_v.alloc(blocks + 1));
    KCHECK(d_first_t.alloc(blocks + 1));
    KCHECK(hipMemcpy(d_vol.p, v->data, total * sizeof(S), hipMemcpyHostToDevice));
    KCHECK(hipMemsetAsync(d_count_v.p + blocks, 0, sizeof(unsigned long long), 0));
    KCHECK(hipMemsetAsync(d_count_t.p + blocks, 0, sizeof(unsigned long long), 0));
    hipError_t e = chunked_launch(total, [&](unsigned n, size_t base) {
        iso_classify_kernel<S><<<n, ISO_BLOCK>>>(base, d_vol.p, total, p, d_mask.p, d_config.p, d_count_v.p, d_count_t.p);
    });
    if (e != hipSuccess) return hip_fail("frog_isosurface_create: classify", e);
    uint64_t n_v = 0, n_t = 0;
    if (int rc = iso_block_offsets(d_count_v, d_first_v, blocks, d_temp, &n_v)) return rc;
    if (int rc = iso_block_offsets(d_count_t, d_first_t, blocks, d_temp, &n_t)) return rc;
    if (n_v >= iso_result_max() || n_t >= iso_result_max())
        return fail(FROG_E_INVALID, "frog_isosurface_create: " + std::to_string(n_v) + " vertices and " + std::to_string(n_t) +
                                        " triangles: a surface holds fewer than " + std::to_string(iso_result_max()) + " of each");
    if (!n_v) return FROG_OK;
    frog::DevBuf<uint32_t> d_vertex_offset;
    KCHECK(d_vertex_offset.alloc(total));
    KCHECK(s->d_xyz.alloc(3 * (size_t)n_v));
    KCHECK(s->d_triangles.alloc(3 * (size_t)n_t));
    e = chunked_launch(total, [&](unsigned n, size_t base) {
        iso_vertices_kernel<S><<<n, ISO_BLOCK>>>(base, d_vol.p, total, p, d_mask.p, d_first_v.p, d_vertex_offset.p, s->d_xyz.p);
    });
    if (e == hipSuccess && n_t) {
        e = chunked_launch(total, [&](unsigned n, size_t base) {
            iso_triangles_kernel<<<n, ISO_BLOCK>>>(base, total, p.g, d_mask.p, d_config.p, d_first_t.p, d_vertex_offset.p, s->d_triangles.p);
        });
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("frog_isosurface_create: emit", e);
    s->n_vertices = (uint32_t)n_v;
    s->n_triangles = (uint32_t)n_t;
    return FROG_OK;
}

// ---- mesh filters (k_mesh.hip.h) --------------------------------------------------------------------------------------------------

// The largest mesh the smoothing accepts: its adjacency sorts two 64-bit keys per face index, and hipcub's run-length pass counts
// its items in a signed 32-bit integer.
constexpr uint64_t MESH_MAX_POINTS = ((uint64_t)1 << 31) - 1;
constexpr uint64_t MESH_MAX_INDICES = ((uint64_t)1 << 30) - 1;

// floats per vertex of the passes' working copies: 3 (the mesh's own packed rows, smoothed in place against one second buffer)
// or 4 (16-byte rows, one load per neighbour, padded in and out).  The two give the same bytes; DESIGN 31 measured the packed
// rows faster, in the pass kernel and in the whole call, and FROG_MESH_STRIDE=3 or 4 chooses one of them.
constexpr int MESH_STRIDE_DEFAULT = 3;

int mesh_stride()
{
    static const int stride = [] {
        const char *s = getenv("FROG_MESH_STRIDE");
        const int v = s ? atoi(s) : 0;
        return v == 3 || v == 4 ? v : MESH_STRIDE_DEFAULT;
    }();
    return stride;
}

int bit_length(uint64_t v)
{
    int bits = 0;
    for (; v; v >>= 1) bits++;
    return bits;
}

int mesh_smooth_arguments(const char *where, double lambda, double mu, int boundary)
{
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return fail(FROG_E_INVALID, std::string(where) + ": lambda and mu are finite");
    if (boundary != 0 && boundary != 1) return fail(FROG_E_INVALID, std::string(where) + ": boundary 0 or 1");
    return FROG_OK;
}

// host arrays: every one of the count indices is below n
int mesh_indices_below(const char *where, const uint32_t *idx, size_t count, uint64_t n)
{
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= n) return fail(FROG_E_INVALID, std::string(where) + ": face index " + std::to_string(idx[i]) + " with " + std::to_string(n) + " points");
    return FROG_OK;
}

// the CSR of the header's N(v): ptr[n + 1], col[n_entries]
struct MeshGraph {
    frog::DevBuf<uint32_t> d_ptr, d_col;
    uint32_t n_entries = 0;
};

// d_face_ptr == nullptr: triangles.  n > 0, 0 < n_indices <= MESH_MAX_INDICES.
int mesh_graph_build(size_t n, const uint32_t *d_face_ptr, const uint32_t *d_face_idx, size_t n_faces, size_t n_indices, int boundary, MeshGraph &g)
{
    const size_t slots = 2 * n_indices;
    frog::DevBuf<unsigned long long> d_keys, d_sorted;
    frog::DevBuf<uint32_t> d_times, d_runs, d_raw, d_degree;
    frog::DevBuf<unsigned char> d_temp;
    KCHECK(d_keys.alloc(slots));
    KCHECK(d_sorted.alloc(slots));
    KCHECK(d_times.alloc(slots));
    KCHECK(d_runs.alloc(1));
    hipError_t e = chunked_launch(n_faces, [&](unsigned blocks, size_t base) {
        mesh_edge_keys_kernel<<<blocks, MESH_BLOCK>>>(base, d_face_ptr, d_face_idx, n_faces, (uint32_t)n, d_keys.p);
    });
    if (e != hipSuccess) return hip_fail("mesh adjacency: keys", e);
    const int end_bit = 32 + bit_length(n);             // the sentinel n << 32 | n included
    size_t bytes = 0;
    KCHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, d_keys.p, d_sorted.p, slots, 0, end_bit));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceRadixSort::SortKeys(d_temp.p, bytes, d_keys.p, d_sorted.p, slots, 0, end_bit));
    // the distinct keys go where the unsorted ones were
    bytes = 0;
    KCHECK(hipcub::DeviceRunLengthEncode::Encode(nullptr, bytes, d_sorted.p, d_keys.p, d_times.p, d_runs.p, (int)slots));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceRunLengthEncode::Encode(d_temp.p, bytes, d_sorted.p, d_keys.p, d_times.p, d_runs.p, (int)slots));
    uint32_t runs = 0;
    KCHECK(hipMemcpy(&runs, d_runs.p, sizeof runs, hipMemcpyDeviceToHost));
    unsigned long long last_key = 0;
    if (runs) KCHECK(hipMemcpy(&last_key, d_keys.p + (runs - 1), sizeof last_key, hipMemcpyDeviceToHost));
    const uint32_t raw_entries = runs && last_key == ((unsigned long long)n << 32 | n) ? runs - 1 : runs;

    KCHECK(d_raw.alloc(n + 1));
    KCHECK(d_degree.alloc(n + 1));
    KCHECK(g.d_ptr.alloc(n + 1));
    e = chunked_launch(n + 1, [&](unsigned blocks, size_t base) {
        mesh_row_kernel<<<blocks, MESH_BLOCK>>>(base, d_keys.p, raw_entries, n, d_raw.p);
    });
    if (e == hipSuccess) {
        e = chunked_launch(n + 1, [&](unsigned blocks, size_t base) {
            mesh_degree_kernel<<<blocks, MESH_BLOCK>>>(base, d_raw.p, d_keys.p, d_times.p, n, boundary, d_degree.p);
        });
    }
    if (e != hipSuccess) return hip_fail("mesh adjacency: rows", e);
    bytes = 0;
    KCHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_degree.p, g.d_ptr.p, n + 1));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceScan::ExclusiveSum(d_temp.p, bytes, d_degree.p, g.d_ptr.p, n + 1));
    KCHECK(hipMemcpy(&g.n_entries, g.d_ptr.p + n, sizeof g.n_entries, hipMemcpyDeviceToHost));
    if (!g.n_entries) return FROG_OK;
    KCHECK(g.d_col.alloc(g.n_entries));
    e = chunked_launch(n, [&](unsigned blocks, size_t base) {
        mesh_fill_kernel<<<blocks, MESH_BLOCK>>>(base, d_raw.p, d_keys.p, d_times.p, n, boundary, g.d_ptr.p, g.d_col.p);
    });
    if (e == hipSuccess) e = hipDeviceSynchronize();        // the build's buffers are freed on return
    if (e != hipSuccess) return hip_fail("mesh adjacency: fill", e);
    return FROG_OK;
}

template <int STRIDE>
hipError_t mesh_pass(size_t n, const MeshGraph &g, const float *from, float *to, double f)
{
    return chunked_launch(n, [&](unsigned blocks, size_t base) {
        mesh_pass_kernel<STRIDE><<<blocks, MESH_BLOCK>>>(base, n, g.d_ptr.p, g.d_col.p, from, to, f);
    });
}

// 2 x iterations passes over the graph on d_xyz (3 floats per vertex, on the current device); the result is back in d_xyz
int mesh_passes(float *d_xyz, size_t n, const MeshGraph &g, uint32_t iterations, double lambda, double mu)
{
    const int stride = mesh_stride();
    frog::DevBuf<float> d_a, d_b;
    float *from = d_xyz, *to = nullptr;
    hipError_t e = hipSuccess;
    KCHECK(d_b.alloc((size_t)stride * n));
    to = d_b.p;
    if (stride == 4) {
        KCHECK(d_a.alloc(4 * n));
        from = d_a.p;
        e = chunked_launch(n, [&](unsigned blocks, size_t base) { mesh_pad_kernel<<<blocks, MESH_BLOCK>>>(base, d_xyz, d_a.p, n); });
    }
    for (uint32_t it = 0; it < 2 * (uint64_t)iterations && e == hipSuccess; it++) {
        const double f = it % 2 ? mu : lambda;
        e = stride == 4 ? mesh_pass<4>(n, g, from, to, f) : mesh_pass<3>(n, g, from, to, f);
        std::swap(from, to);
    }
    // an even number of passes: the result lies where the first pass read
    if (e == hipSuccess && stride == 4)
        e = chunked_launch(n, [&](unsigned blocks, size_t base) { mesh_unpad_kernel<<<blocks, MESH_BLOCK>>>(base, d_a.p, d_xyz, n); });
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("mesh smoothing: passes", e);
    return FROG_OK;
}

// frog_mesh_smooth and frog_isosurface_smooth after their argument checks, on the current device
int mesh_smooth_device(const char *where, float *d_xyz, size_t n, const uint32_t *d_face_ptr, const uint32_t *d_face_idx, size_t n_faces,
                       size_t n_indices, uint32_t iterations, double lambda, double mu, int boundary)
{
    if (n > MESH_MAX_POINTS || n_indices > MESH_MAX_INDICES)
        return fail(FROG_E_INVALID, std::string(where) + ": " + std::to_string(n) + " points and " + std::to_string(n_indices) +
                                        " face indices: at most " + std::to_string(MESH_MAX_POINTS) + " and " + std::to_string(MESH_MAX_INDICES));
    if (!n || !n_indices || !iterations || (lambda == 0.0 && mu == 0.0)) return FROG_OK;
    if (iterations > ((uint32_t)1 << 30)) return fail(FROG_E_INVALID, std::string(where) + ": at most 2^30 iterations");
    MeshGraph g;
    if (int rc = mesh_graph_build(n, d_face_ptr, d_face_idx, n_faces, n_indices, boundary, g)) return rc;
    if (!g.n_entries) return FROG_OK;
    return mesh_passes(d_xyz, n, g, iterations, lambda, mu);
}

// frog_isosurface_cluster on the current device; cell is a finite double > 0 and the mesh has a vertex
int mesh_cluster_device(frog_isosurface *s, double cell, uint32_t *cluster_of)
{
    const size_t n = s->n_vertices, m = s->n_triangles;
    const int bound_blocks = (int)std::min<size_t>(MESH_BOUNDS_BLOCKS, (n + MESH_BLOCK - 1) / MESH_BLOCK);
    frog::DevBuf<MeshBounds> d_partial, d_bounds;
    KCHECK(d_partial.alloc(bound_blocks));
    KCHECK(d_bounds.alloc(1));
    mesh_bounds_kernel<<<bound_blocks, MESH_BLOCK>>>(s->d_xyz.p, n, d_partial.p);
    mesh_bounds_final_kernel<<<1, MESH_BLOCK>>>(d_partial.p, bound_blocks, d_bounds.p);
    KCHECK(hipGetLastError());
    MeshBounds b;
    KCHECK(hipMemcpy(&b, d_bounds.p, sizeof b, hipMemcpyDeviceToHost));
    if (b.bad) return fail(FROG_E_INVALID, "frog_isosurface_cluster: " + std::to_string(b.bad) + " coordinates are not finite");
    MeshCells cells;
    cells.cell = cell;
    for (int k = 0; k < 3; k++) {
        cells.lo[k] = (double)b.lo[k];
        const double top = std::floor(((double)b.hi[k] - (double)b.lo[k]) / cell);      // the largest c on this axis: c ascends with x
        if (!(top < 2097152.0)) return fail(FROG_E_INVALID, "frog_isosurface_cluster: more than 2^21 cells on an axis");
        cells.count[k] = (unsigned long long)top + 1;
    }

    frog::DevBuf<unsigned long long> d_keys, d_sorted;
    frog::DevBuf<uint32_t> d_order, d_members, d_times, d_first, d_runs, d_cluster_of, d_new_triangles;
    frog::DevBuf<float> d_new_xyz;
    frog::DevBuf<unsigned char> d_temp;
    KCHECK(d_keys.alloc(n));
    KCHECK(d_sorted.alloc(n));
    KCHECK(d_order.alloc(n));
    KCHECK(d_members.alloc(n));
    KCHECK(d_times.alloc(n + 1));
    KCHECK(d_first.alloc(n + 1));
    KCHECK(d_runs.alloc(1));
    KCHECK(d_cluster_of.alloc(n));
    hipError_t e = chunked_launch(n, [&](unsigned blocks, size_t base) {
        mesh_cell_keys_kernel<<<blocks, MESH_BLOCK>>>(base, s->d_xyz.p, n, cells, d_keys.p, d_order.p);
    });
    if (e != hipSuccess) return hip_fail("frog_isosurface_cluster: keys", e);
    const int end_bit = std::max(1, bit_length(cells.count[0] * cells.count[1] * cells.count[2] - 1));      // <= 2^63 cells
    size_t bytes = 0;
    KCHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, d_keys.p, d_sorted.p, d_order.p, d_members.p, n, 0, end_bit));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceRadixSort::SortPairs(d_temp.p, bytes, d_keys.p, d_sorted.p, d_order.p, d_members.p, n, 0, end_bit));
    bytes = 0;
    KCHECK(hipcub::DeviceRunLengthEncode::Encode(nullptr, bytes, d_sorted.p, d_keys.p, d_times.p, d_runs.p, (int)n));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceRunLengthEncode::Encode(d_temp.p, bytes, d_sorted.p, d_keys.p, d_times.p, d_runs.p, (int)n));
    uint32_t n_clusters = 0;
    KCHECK(hipMemcpy(&n_clusters, d_runs.p, sizeof n_clusters, hipMemcpyDeviceToHost));
    KCHECK(hipMemsetAsync(d_times.p + n_clusters, 0, sizeof(uint32_t), 0));
    bytes = 0;
    KCHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_times.p, d_first.p, (size_t)n_clusters + 1));
    KCHECK(d_temp.alloc(std::max<size_t>(bytes, 1)));
    KCHECK(hipcub::DeviceScan::ExclusiveSum(d_temp.p, bytes, d_times.p, d_first.p, (size_t)n_clusters + 1));
    KCHECK(d_new_xyz.alloc(3 * (size_t)n_clusters));
    e = chunked_launch(n_clusters, [&](unsigned blocks, size_t base) {
        mesh_cluster_kernel<<<blocks, MESH_BLOCK>>>(base, s->d_xyz.p, d_members.p, d_first.p, n_clusters, d_new_xyz.p, d_cluster_of.p);
    });
    if (e != hipSuccess) return hip_fail("frog_isosurface_cluster: means", e);

    uint64_t kept = 0;
    if (m) {
        const size_t blocks = (m + MESH_BLOCK - 1) / MESH_BLOCK;
        frog::DevBuf<unsigned long long> d_count, d_offset;
        KCHECK(d_count.alloc(blocks + 1));
        KCHECK(d_offset.alloc(blocks + 1));
        KCHECK(hipMemsetAsync(d_count.p + blocks, 0, sizeof(unsigned long long), 0));
        e = chunked_launch(m, [&](unsigned nb, size_t base) {
            mesh_triangle_count_kernel<<<nb, MESH_BLOCK>>>(base, s->d_triangles.p, d_cluster_of.p, m, d_count.p);
        });
        if (e != hipSuccess) return hip_fail("frog_isosurface_cluster: count", e);
        if (int rc = iso_block_offsets(d_count, d_offset, blocks, d_temp, &kept)) return rc;
        if (kept) {
            KCHECK(d_new_triangles.alloc(3 * (size_t)kept));
            e = chunked_launch(m, [&](unsigned nb, size_t base) {
                mesh_triangle_emit_kernel<<<nb, MESH_BLOCK>>>(base, s->d_triangles.p, d_cluster_of.p, m, d_offset.p, d_new_triangles.p);
            });
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();    // d_count and d_offset go out of scope
        if (e != hipSuccess) return hip_fail("frog_isosurface_cluster: triangles", e);
    }
    if (cluster_of) KCHECK(hipMemcpy(cluster_of, d_cluster_of.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    KCHECK(hipDeviceSynchronize());
    s->d_xyz.swap(d_new_xyz);
    s->d_triangles.swap(d_new_triangles);
    s->n_vertices = n_clusters;
    s->n_triangles = (uint32_t)kept;
    return FROG_OK;
}

} // namespace

extern "C" {

int frog_chain_create(const frog_chain_link *links, uint32_t n_links, int device, frog_chain **out)
{
    if (!out || (n_links && !links)) return fail(FROG_E_INVALID, "bad arguments to frog_chain_create");
    if (int rc = select_device(device)) return rc;
    std::unique_ptr<frog_chain> c(new (std::nothrow) frog_chain);
    if (!c) return fail(FROG_E_NOMEM, "out of host memory");
    c->device = device;
    for (uint32_t l = 0; l < n_links; l++) {
        const frog_chain_link &t = links[l];
        DevLink d;
        std::memset(&d, 0, sizeof d);
        d.type = t.type;
        if (t.type == FROG_T_LINEAR) {
            for (int k = 0; k < 12; k++) d.m[k] = t.matrix[k];
        } else if (t.type == FROG_T_BSPLINE || t.type == FROG_T_BSPLINE_INVERSE || t.type == FROG_T_FIELD) {
            // a field's nodes are validated and uploaded like a lattice's control points
            const size_t G = (size_t)t.dims[0] * t.dims[1] * t.dims[2];
            if (!G || !t.coeffs) return fail(FROG_E_INVALID, "empty lattice");
            for (int k = 0; k < 3; k++) {
                if (!(t.spacing[k] > 0)) return fail(FROG_E_INVALID, "lattice spacing must be positive");
                d.dims[k] = (int)t.dims[k]; d.origin[k] = t.origin[k]; d.spacing[k] = t.spacing[k];
            }
            frog::DevBuf<float> &coeffs = c->d_coeffs.emplace_back();
            hipError_t e = coeffs.alloc(3 * G);
            if (e == hipSuccess) e = hipMemcpy(coeffs.p, t.coeffs, 3 * G * sizeof(float), hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_fail("cannot copy lattice coefficients to the device", e);
            d.coeffs = coeffs.p;
        } else {
            return fail(FROG_E_INVALID, "unknown transform type");
        }
        c->h_links.push_back(d);
    }
    if (n_links) {
        hipError_t e = c->d_links.alloc(n_links);
        if (e == hipSuccess) e = hipMemcpy(c->d_links.p, c->h_links.data(), n_links * sizeof(DevLink), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail("cannot copy the chain to the device", e);
    }
    *out = c.release();
    return FROG_OK;
}

void frog_chain_destroy(frog_chain *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

uint32_t frog_chain_num_links(const frog_chain *c) { return c ? (uint32_t)c->h_links.size() : 0; }

int frog_chain_apply(frog_chain *c, const double *in, double *out, size_t n)
{
    if (!c || (n && (!in || !out))) return fail(FROG_E_INVALID, "bad arguments to frog_chain_apply");
    if (!n) return FROG_OK;
    KCHECK(hipSetDevice(c->device));
    frog::DevBuf<double> d_in, d_out;
    KCHECK(d_in.alloc(3 * n));
    KCHECK(d_out.alloc(3 * n));
    hipError_t e = hipMemcpy(d_in.p, in, 3 * n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        e = chunked_launch(n, [&](unsigned blocks, size_t base) {
            chain_apply_kernel<<<blocks, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), d_in.p, d_out.p, n);
        });
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_chain_apply", e);
    return FROG_OK;
}

int frog_chain_apply_f32(frog_chain *c, const float *in, float *out, size_t n)
{
    if (!c || (n && (!in || !out))) return fail(FROG_E_INVALID, "bad arguments to frog_chain_apply_f32");
    if (!n) return FROG_OK;
    KCHECK(hipSetDevice(c->device));
    frog::DevBuf<float> d_p;
    KCHECK(d_p.alloc(3 * n));
    hipError_t e = hipMemcpy(d_p.p, in, 3 * n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = chain_apply_f32_device(c, d_p.p, d_p.p, n);
    if (e == hipSuccess) e = hipMemcpy(out, d_p.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_chain_apply_f32", e);
    return FROG_OK;
}

int frog_isosurface_create(const frog_volume *volume, int mode, double level, int64_t value, int device,
                           frog_isosurface **out, uint32_t *n_vertices, uint32_t *n_triangles)
{
    if (!volume || !volume->data || !out || !n_vertices || !n_triangles) return fail(FROG_E_INVALID, "bad arguments to frog_isosurface_create");
    if (mode != FROG_ISO_LEVEL && mode != FROG_ISO_LABEL) return fail(FROG_E_INVALID, "frog_isosurface_create: mode FROG_ISO_LEVEL or FROG_ISO_LABEL");
    if (!frog_volume_voxel_bytes(volume->dtype)) return fail(FROG_E_INVALID, "frog_isosurface_create: unknown scalar type");
    if (mode == FROG_ISO_LABEL && !integer_voxel_type(volume->dtype))
        return fail(FROG_E_INVALID, "frog_isosurface_create: a label volume has an integer type");
    if (mode == FROG_ISO_LEVEL && std::isnan(level)) return fail(FROG_E_INVALID, "frog_isosurface_create: the level is NaN");
    const uint64_t slice = (uint64_t)volume->dims[0] * volume->dims[1];         // < 2^64
    if (slice > ((uint64_t)1 << 31) || slice * volume->dims[2] > ((uint64_t)1 << 31))
        return fail(FROG_E_INVALID, "frog_isosurface_create: more than 2^31 nodes");
    if (int rc = select_device(device)) return rc;
    std::unique_ptr<frog_isosurface> s(new (std::nothrow) frog_isosurface);
    if (!s) return fail(FROG_E_NOMEM, "out of host memory");
    s->device = device;
    if (volume->dims[0] >= 2 && volume->dims[1] >= 2 && volume->dims[2] >= 2) {
        const size_t total = voxel_count(volume);
        if (int rc = with_voxel_type(volume->dtype, [&](auto t) { return isosurface_typed<decltype(t)>(s.get(), volume, total, mode, level, (long long)value); }))
            return rc;
    }
    *n_vertices = s->n_vertices;
    *n_triangles = s->n_triangles;
    *out = s.release();
    return FROG_OK;
}

int frog_isosurface_apply(frog_isosurface *s, frog_chain *c)
{
    if (!s || !c) return fail(FROG_E_INVALID, "bad arguments to frog_isosurface_apply");
    if (c->device != s->device) return fail(FROG_E_INVALID, "frog_isosurface_apply: the chain is on another device");
    if (!s->n_vertices) return FROG_OK;
    KCHECK(hipSetDevice(s->device));
    hipError_t e = chain_apply_f32_device(c, s->d_xyz.p, s->d_xyz.p, s->n_vertices);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("frog_isosurface_apply", e);
    return FROG_OK;
}

int frog_isosurface_get(frog_isosurface *s, float *xyz, uint32_t *triangles)
{
    if (!s || (s->n_vertices && !xyz) || (s->n_triangles && !triangles)) return fail(FROG_E_INVALID, "bad arguments to frog_isosurface_get");
    KCHECK(hipSetDevice(s->device));
    if (s->n_vertices) KCHECK(hipMemcpy(xyz, s->d_xyz.p, 3 * (size_t)s->n_vertices * sizeof(float), hipMemcpyDeviceToHost));
    if (s->n_triangles) KCHECK(hipMemcpy(triangles, s->d_triangles.p, 3 * (size_t)s->n_triangles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FROG_OK;
}

void frog_isosurface_destroy(frog_isosurface *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int frog_mesh_smooth(float *xyz, size_t n_points, const uint32_t *face_ptr, const uint32_t *face_idx, size_t n_faces,
                     uint32_t iterations, double lambda, double mu, int boundary, int device)
{
    const char *where = "frog_mesh_smooth";
    if ((n_points && !xyz) || (n_faces && !face_ptr)) return fail(FROG_E_INVALID, "bad arguments to frog_mesh_smooth");
    if (int rc = mesh_smooth_arguments(where, lambda, mu, boundary)) return rc;
    if (n_faces >= ((uint64_t)1 << 32)) return fail(FROG_E_INVALID, "frog_mesh_smooth: more than 2^32 - 1 faces");
    size_t n_indices = 0;
    if (n_faces) {
        if (face_ptr[0] != 0) return fail(FROG_E_INVALID, "frog_mesh_smooth: face_ptr starts at 0");
        for (size_t f = 0; f < n_faces; f++)
            if (face_ptr[f + 1] < face_ptr[f]) return fail(FROG_E_INVALID, "frog_mesh_smooth: face_ptr descends");
        n_indices = face_ptr[n_faces];
    }
    if (n_indices && !face_idx) return fail(FROG_E_INVALID, "bad arguments to frog_mesh_smooth");
    if (int rc = mesh_indices_below(where, face_idx, n_indices, n_points)) return rc;
    if (n_points > MESH_MAX_POINTS || n_indices > MESH_MAX_INDICES)
        return fail(FROG_E_INVALID, "frog_mesh_smooth: at most " + std::to_string(MESH_MAX_POINTS) + " points and " +
                                        std::to_string(MESH_MAX_INDICES) + " face indices");
    if (int rc = select_device(device)) return rc;
    if (!n_points || !n_indices) return FROG_OK;
    frog::DevBuf<float> d_xyz;
    frog::DevBuf<uint32_t> d_ptr, d_idx;
    KCHECK(d_xyz.alloc(3 * n_points));
    KCHECK(d_ptr.alloc(n_faces + 1));
    KCHECK(d_idx.alloc(n_indices));
    KCHECK(hipMemcpy(d_xyz.p, xyz, 3 * n_points * sizeof(float), hipMemcpyHostToDevice));
    KCHECK(hipMemcpy(d_ptr.p, face_ptr, (n_faces + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    KCHECK(hipMemcpy(d_idx.p, face_idx, n_indices * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int rc = mesh_smooth_device(where, d_xyz.p, n_points, d_ptr.p, d_idx.p, n_faces, n_indices, iterations, lambda, mu, boundary)) return rc;
    KCHECK(hipMemcpy(xyz, d_xyz.p, 3 * n_points * sizeof(float), hipMemcpyDeviceToHost));
    return FROG_OK;
}

int frog_isosurface_smooth(frog_isosurface *s, uint32_t iterations, double lambda, double mu, int boundary)
{
    if (!s) return fail(FROG_E_INVALID, "bad arguments to frog_isosurface_smooth");
    if (int rc = mesh_smooth_arguments("frog_isosurface_smooth", lambda, mu, boundary)) return rc;
    KCHECK(hipSetDevice(s->device));
    return mesh_smooth_device("frog_isosurface_smooth", s->d_xyz.p, s->n_vertices, nullptr, s->d_triangles.p, s->n_triangles,
                              3 * (size_t)s->n_triangles, iterations, lambda, mu, boundary);
}

int frog_isosurface_upload(const float *xyz, uint32_t n, const uint32_t *triangles, uint32_t m, int device, frog_isosurface **out)
{
    if (!out || (n && !xyz) || (m && !triangles)) return fail(FROG_E_INVALID, "bad arguments to frog_isosurface_upload");
    if (n >= ((uint32_t)1 << 31) || m >= ((uint32_t)1 << 31))
        return fail(FROG_E_INVALID, "frog_isosurface_upload: a surface holds fewer than 2^31 vertices and triangles");
    if (int rc = mesh_indices_below("frog_isosurface_upload", triangles, 3 * (size_t)m, n)) return rc;
    if (int rc = select_device(device)) return rc;
    std::unique_ptr<frog_isosurface> s(new (std::nothrow) frog_isosurface);
    if (!s) return fail(FROG_E_NOMEM, "out of host memory");
    s->device = device;
    KCHECK(s->d_xyz.alloc(3 * (size_t)n));
    KCHECK(s->d_triangles.alloc(3 * (size_t)m));
    if (n) KCHECK(hipMemcpy(s->d_xyz.p, xyz, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (m) KCHECK(hipMemcpy(s->d_triangles.p, triangles, 3 * (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice));
    s->n_vertices = n;
    s->n_triangles = m;
    *out = s.release();
    return FROG_OK;
}

int frog_isosurface_cluster(frog_isosurface *s, double cell, uint32_t *n_vertices, uint32_t *n_triangles, uint32_t *cluster_of)
{
    if (!s || !n_vertices || !n_triangles) return fail(FROG_E_INVALID, "bad arguments to frog_isosurface_cluster");
    if (!(std::isfinite(cell) && cell > 0.0)) return fail(FROG_E_INVALID, "frog_isosurface_cluster: the cell is a finite size > 0");
    if (s->n_vertices) {
        KCHECK(hipSetDevice(s->device));
        if (int rc = mesh_cluster_device(s, cell, cluster_of)) return rc;
    }
    *n_vertices = s->n_vertices;
    *n_triangles = s->n_triangles;
    return FROG_OK;
}

int frog_chain_check(frog_chain *c, const double origin[3], const double spacing[3], const uint32_t dims[3],
                     uint64_t *n_negative, double *min_determinant)
{
    if (!c || !origin || !spacing || !dims || !n_negative) return fail(FROG_E_INVALID, "bad arguments to frog_chain_check");
    const size_t total = (size_t)dims[0] * dims[1] * dims[2];
    *n_negative = 0;
    if (min_determinant) *min_determinant = INFINITY;
    if (!total) return FROG_OK;
    if (total > ((size_t)1 << 40)) return fail(FROG_E_INVALID, "grid too large");
    KCHECK(hipSetDevice(c->device));
    const size_t blocks = (total + LAUNCH_BLOCK - 1) / LAUNCH_BLOCK;     // one block_min slot per block of the whole grid
    frog::DevBuf<unsigned long long> d_neg;
    frog::DevBuf<double> d_min;
    KCHECK(d_neg.alloc(1));
    KCHECK(d_min.alloc(blocks));
    hipError_t e = hipMemset(d_neg.p, 0, sizeof(unsigned long long));
    if (e == hipSuccess) {
        const NodeGrid grid = node_grid(origin, spacing, dims);
        e = chunked_launch(total, [&](unsigned nb, size_t base) {
            chain_check_kernel<<<nb, LAUNCH_BLOCK>>>(base, c->d_links.p, (int)c->h_links.size(), grid, d_neg.p, d_min.p);
        });
    }
    unsigned long long neg = 0;
    std::vector<double> mins(blocks);
    if (e == hipSuccess) e = hipMemcpy(&neg, d_neg.p, sizeof neg, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mins.data(), d_min.p, blocks * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_chain_check", e);
    *n_negative = neg;
    if (min_determinant) { double m = INFINITY; for (double v : mins) m = std::fmin(m, v); *min_determinant = m; }
    return FROG_OK;
}

int frog_chain_invert_links(const frog_chain_link *in, uint32_t n, frog_chain_link *out)
{
    if (n && (!in || !out)) return fail(FROG_E_INVALID, "bad arguments to frog_chain_invert_links");
    for (uint32_t l = 0; l < n; l++) {
        frog_chain_link t = in[n - 1 - l];
        if (t.type == FROG_T_BSPLINE) t.type = FROG_T_BSPLINE_INVERSE;
        else if (t.type == FROG_T_BSPLINE_INVERSE) t.type = FROG_T_BSPLINE;
        else if (t.type == FROG_T_LINEAR) {
            // affine inverse: [A b; 0 1]^-1 = [A^-1  -A^-1 b; 0 1]
            const double *m = in[n - 1 - l].matrix;
            const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
            const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
            const double det = a00 * c00 + a01 * c01 + a02 * c02;
            if (det == 0.0 || !std::isfinite(det)) return fail(FROG_E_INVALID, "singular matrix in the chain");
            double inv[3][3] = {
                { c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det },
                { c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det },
                { c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det } };
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) t.matrix[4 * r + c] = inv[r][c];
                t.matrix[4 * r + 3] = -(inv[r][0] * m[3] + inv[r][1] * m[7] + inv[r][2] * m[11]);
            }
            t.matrix[12] = t.matrix[13] = t.matrix[14] = 0.0; t.matrix[15] = 1.0;
        } else if (t.type == FROG_T_FIELD) {
            return fail(FROG_E_INVALID, "a displacement field link has no inverse form: sample the inverted chain instead");
        } else {
            return fail(FROG_E_INVALID, "unknown transform type");
        }
        out[l] = t;
    }
    return FROG_OK;
}

int frog_chain_sample(frog_chain *c, const double origin[3], const double spacing[3], const uint32_t dims[3],
                      int dtype, void *displacement, void *determinant)
{
    if (!c || !origin || !spacing || !dims) return fail(FROG_E_INVALID, "bad arguments to frog_chain_sample");
    if (!displacement && !determinant) return fail(FROG_E_INVALID, "frog_chain_sample: no output asked for");
    if (dtype != FROG_V_F32 && dtype != FROG_V_F64) return fail(FROG_E_INVALID, "frog_chain_sample: the output type must be FROG_V_F32 or FROG_V_F64");
    const size_t limit = (size_t)1 << 40, plane = (size_t)dims[0] * dims[1];
    if (!plane || !dims[2]) return FROG_OK;
    if (plane > limit || dims[2] > limit / plane) return fail(FROG_E_INVALID, "grid too large");
    const size_t total = plane * dims[2];
    KCHECK(hipSetDevice(c->device));
    const NodeGrid grid = node_grid(origin, spacing, dims);
    if (dtype == FROG_V_F32) return sample_typed<float>(c, grid, total, (float *)displacement, (float *)determinant);
    return sample_typed<double>(c, grid, total, (double *)displacement, (double *)determinant);
}

int frog_chain_reslice(frog_chain *c, const frog_volume *src, frog_volume *out, int interpolation, double background)
{
    if (!c || !src || !out || !src->data || !out->data) return fail(FROG_E_INVALID, "bad arguments to frog_chain_reslice");
    if (out->dtype != src->dtype || !frog_volume_voxel_bytes(src->dtype)) return fail(FROG_E_INVALID, "output and source scalar types must match");
    if (!voxel_count(src) || !voxel_count(out)) return fail(FROG_E_INVALID, "empty volume");
    if (!chain_samples(src)) return fail(FROG_E_INVALID, "bad source geometry");
    KCHECK(hipSetDevice(c->device));
    return with_voxel_type(src->dtype, [&](auto s) { return reslice_typed<decltype(s)>(c, src, out, interpolation, background); });
}

int frog_average_create(const frog_volume *grid, uint32_t n_images, int device, frog_average **out)
{
    size_t total;
    if (int rc = group_arguments("frog_average_create", grid, out, &total)) return rc;
    if (!n_images) return fail(FROG_E_INVALID, "bad arguments to frog_average_create");
    std::unique_ptr<frog_average> a;
    if (int rc = group_new(grid, total, device, a)) return rc;
    a->n_images = n_images;
    KCHECK(a->d_avg.alloc(total));
    KCHECK(a->d_sq.alloc(total));
    // both accumulators start at zero (the reference never clears its stdev image: AverageVolumes.cxx:31-43)
    KCHECK(hipMemset(a->d_avg.p, 0, total * sizeof(float)));
    KCHECK(hipMemset(a->d_sq.p, 0, total * sizeof(float)));
    *out = a.release();
    return FROG_OK;
}

int frog_average_add(frog_average *a, frog_chain *c, const frog_volume *src, int interpolation, double background, frog_volume *resliced)
{
    if (!a || !src || !src->data || !frog_volume_voxel_bytes(src->dtype)) return fail(FROG_E_INVALID, "bad arguments to frog_average_add");
    if (a->finished || a->added >= a->n_images) return fail(FROG_E_INVALID, "frog_average_add: more volumes than n_images");
    if (int rc = add_inputs("frog_average_add", a, c, src, resliced)) return rc;
    KCHECK(hipSetDevice(a->device));
    const int rc = with_voxel_type(src->dtype, [&](auto s) { return average_add_typed<decltype(s)>(a, c, src, interpolation, background, resliced); });
    if (rc == FROG_OK) a->added++;
    return rc;
}

int frog_average_finish(frog_average *a, float *mean, float *stdev)
{
    if (!a || !mean || !stdev) return fail(FROG_E_INVALID, "bad arguments to frog_average_finish");
    if (a->added != a->n_images) return fail(FROG_E_INVALID, "frog_average_finish: fewer volumes added than n_images");
    KCHECK(hipSetDevice(a->device));
    hipError_t e = hipSuccess;
    if (!a->finished) {
        e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
            average_finish_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_avg.p, a->d_sq.p, a->total);
        });
        a->finished = e == hipSuccess;                 // stdev now stands in place of sq: a second call only copies
    }
    if (e == hipSuccess) e = hipMemcpy(mean, a->d_avg.p, a->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(stdev, a->d_sq.p, a->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_average_finish", e);
    return FROG_OK;
}

void frog_average_destroy(frog_average *a) { group_destroy(a); }

int frog_cover_create(const frog_volume *grid, int device, frog_cover **out)
{
    size_t total;
    if (int rc = group_arguments("frog_cover_create", grid, out, &total)) return rc;
    std::unique_ptr<frog_cover> a;
    if (int rc = group_new(grid, total, device, a)) return rc;
    KCHECK(a->d_mean.alloc(total));
    KCHECK(a->d_m2.alloc(total));
    KCHECK(a->d_count.alloc(total));
    KCHECK(hipMemset(a->d_mean.p, 0, total * sizeof(float)));
    KCHECK(hipMemset(a->d_m2.p, 0, total * sizeof(float)));
    KCHECK(hipMemset(a->d_count.p, 0, total * sizeof(uint16_t)));
    *out = a.release();
    return FROG_OK;
}

int frog_cover_add(frog_cover *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background,
                   frog_volume *resliced)
{
    if (!a || !src || !src->data || !frog_volume_voxel_bytes(src->dtype)) return fail(FROG_E_INVALID, "bad arguments to frog_cover_add");
    if (a->added >= 65535) return fail(FROG_E_INVALID, "frog_cover_add: more than 65535 volumes (16-bit counts)");
    if (int rc = cover_inputs("frog_cover_add", a, c, src, mask, resliced)) return rc;
    if (mask) cover_mask(a, mask);
    KCHECK(hipSetDevice(a->device));
    const int rc = with_voxel_type(src->dtype, [&](auto s) { return cover_add_typed<decltype(s)>(a, c, src, mask, interpolation, background, resliced); });
    if (rc == FROG_OK) a->added++;
    return rc;
}

int frog_cover_score(frog_cover *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background,
                     uint32_t min_count, int leave_one_out, uint32_t bins, float lo, float hi, frog_score_sums *sums, uint64_t *histogram)
{
    if (!a || !src || !src->data || !frog_volume_voxel_bytes(src->dtype) || !sums) return fail(FROG_E_INVALID, "bad arguments to frog_cover_score");
    if (int rc = cover_inputs("frog_cover_score", a, c, src, mask, nullptr)) return rc;
    if (!a->added) return fail(FROG_E_INVALID, "frog_cover_score: before the first frog_cover_add");
    if (!min_count) return fail(FROG_E_INVALID, "frog_cover_score: min_count must be at least 1");
    ScoreParams sp{};
    sp.leave_one_out = leave_one_out != 0;
    sp.need = std::max(sp.leave_one_out ? 2u : 1u, min_count);
    if (bins || histogram) {
        if (!histogram || bins < 2 || bins > 64) return fail(FROG_E_INVALID, "frog_cover_score: 2 to 64 bins and a histogram, or neither");
        const float width = hi - lo;
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo) || !std::isfinite(width))
            return fail(FROG_E_INVALID, "frog_cover_score: the histogram needs a finite range with hi > lo");
        sp.bins = bins;
        sp.lo = lo;
        sp.scale = (float)bins / width;
    }
    if (mask) cover_mask(a, mask);
    KCHECK(hipSetDevice(a->device));
    return with_voxel_type(src->dtype, [&](auto s) { return cover_score_typed<decltype(s)>(a, c, src, mask, interpolation, background, sp, sums, histogram); });
}

int frog_cover_finish(frog_cover *a, uint32_t min_count, float fill, float *mean, float *stdev, uint16_t *count)
{
    if (!a || (!mean && !stdev && !count)) return fail(FROG_E_INVALID, "bad arguments to frog_cover_finish");
    if (!min_count) return fail(FROG_E_INVALID, "frog_cover_finish: min_count must be at least 1");
    if (!a->added) return fail(FROG_E_INVALID, "frog_cover_finish: before the first frog_cover_add");
    KCHECK(hipSetDevice(a->device));
    frog::DevBuf<float> d_mean, d_stdev;
    if (mean) KCHECK(d_mean.alloc(a->total));
    if (stdev) KCHECK(d_stdev.alloc(a->total));
    hipError_t e = hipSuccess;
    if (mean || stdev) {
        e = chunked_launch(a->total, [&](unsigned blocks, size_t base) {
            cover_finish_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_mean.p, a->d_m2.p, a->d_count.p, a->total, min_count, fill, d_mean.p, d_stdev.p);
        });
    }
    if (e == hipSuccess && mean) e = hipMemcpy(mean, d_mean.p, a->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && stdev) e = hipMemcpy(stdev, d_stdev.p, a->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && count) e = hipMemcpy(count, a->d_count.p, a->total * sizeof(uint16_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_cover_finish", e);
    return FROG_OK;
}

void frog_cover_destroy(frog_cover *a) { group_destroy(a); }

int frog_rank_planes(const frog_volume *grid, uint32_t n_images, int device, uint32_t *planes)
{
    size_t total;
    if (int rc = rank_arguments("frog_rank_planes", grid, n_images, planes, &total)) return rc;
    if (int rc = select_device(device)) return rc;
    size_t free_bytes = 0, device_bytes = 0;
    KCHECK(hipMemGetInfo(&free_bytes, &device_bytes));
    const size_t plane_bytes = (size_t)grid->dims[0] * grid->dims[1] * sizeof(uint32_t) * n_images;
    const size_t fit = free_bytes / 2 / plane_bytes;
    if (!fit) return fail(FROG_E_INVALID, "frog_rank_planes: not one plane of the grid fits half of the free device memory");
    *planes = (uint32_t)std::min<size_t>(fit, grid->dims[2]);
    return FROG_OK;
}

int frog_rank_create(const frog_volume *grid, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, int device, frog_rank **out)
{
    size_t total;
    if (int rc = rank_arguments("frog_rank_create", grid, n_images, out, &total)) return rc;
    std::unique_ptr<frog_rank> a;
    if (int rc = windowed_new("frog_rank_create", grid, total, first_plane, n_planes, n_images, device, a)) return rc;
    KCHECK(a->d_keys.alloc((size_t)n_images * a->window));
    *out = a.release();
    return FROG_OK;
}

int frog_rank_add(frog_rank *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background)
{
    return windowed_add<RankEntry>("frog_rank_add", a, a ? a->d_keys.p : nullptr, c, src, mask, interpolation, background);
}

int frog_rank_finish(frog_rank *a, uint32_t min_count, float fill, uint32_t n_q, const double *q, float *quantiles, float *mad, uint16_t *count)
{
    if (!a || n_q > RANK_MAX_Q || (n_q && !q)) return fail(FROG_E_INVALID, "bad arguments to frog_rank_finish");
    if (!min_count) return fail(FROG_E_INVALID, "frog_rank_finish: min_count must be at least 1");
    for (uint32_t j = 0; j < n_q; j++)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail(FROG_E_INVALID, "frog_rank_finish: a probability lies in [0, 1]");
    if (!quantiles) n_q = 0;
    if (!n_q && !mad && !count) return fail(FROG_E_INVALID, "frog_rank_finish: no output asked for");
    if (!a->added) return fail(FROG_E_INVALID, "frog_rank_finish: before the first frog_rank_add");
    KCHECK(hipSetDevice(a->device));
    frog::DevBuf<float> d_q, d_mad;
    frog::DevBuf<uint16_t> d_count;
    if (n_q) KCHECK(d_q.alloc((size_t)n_q * a->window));
    if (mad) KCHECK(d_mad.alloc(a->window));
    if (count) KCHECK(d_count.alloc(a->window));
    RankFinish f{};
    f.window = a->window;
    f.n = a->added;
    f.min_count = min_count;
    f.fill = fill;
    f.n_q = n_q;
    f.sort = n_q || mad;
    for (uint32_t j = 0; j < n_q; j++) f.q[j] = q[j];
    f.quantiles = d_q.p;
    f.mad = d_mad.p;
    f.count = d_count.p;
    hipError_t e = rank_finish_launch(a, f);
    if (e == hipSuccess && n_q) e = hipMemcpy(quantiles, d_q.p, (size_t)n_q * a->window * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mad) e = hipMemcpy(mad, d_mad.p, a->window * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && count) e = hipMemcpy(count, d_count.p, a->window * sizeof(uint16_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_rank_finish", e);
    return FROG_OK;
}

void frog_rank_destroy(frog_rank *a) { group_destroy(a); }

int frog_glm_planes(const frog_volume *grid, uint32_t n_images, int device, uint32_t *planes)
{
    if (n_images > FROG_GLM_MAX_IMAGES) return fail(FROG_E_INVALID, "frog_glm_planes: 1 to " + std::to_string(FROG_GLM_MAX_IMAGES) + " images");
    return frog_rank_planes(grid, n_images, device, planes);       // the same four bytes per image and voxel
}

int frog_glm_create(const frog_volume *grid, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, uint32_t n_columns,
                    const double *design, int device, frog_glm **out)
{
    size_t total;
    if (int rc = group_arguments("frog_glm_create", grid, out, &total)) return rc;
    if (!design) return fail(FROG_E_INVALID, "bad arguments to frog_glm_create");
    if (!n_images || n_images > FROG_GLM_MAX_IMAGES) return fail(FROG_E_INVALID, "frog_glm_create: 1 to " + std::to_string(FROG_GLM_MAX_IMAGES) + " images");
    if (!n_columns || n_columns > FROG_GLM_MAX_COLUMNS) return fail(FROG_E_INVALID, "frog_glm_create: 1 to " + std::to_string(FROG_GLM_MAX_COLUMNS) + " columns");
    if (n_images <= n_columns) return fail(FROG_E_INVALID, "frog_glm_create: more images than columns are needed");
    for (size_t e = 0; e < (size_t)n_images * n_columns; e++)
        if (!std::isfinite(design[e])) return fail(FROG_E_INVALID, "frog_glm_create: a design entry is not finite");
    std::unique_ptr<frog_glm> a;
    if (int rc = windowed_new("frog_glm_create", grid, total, first_plane, n_planes, n_images, device, a)) return rc;
    a->p = n_columns;
    a->design.assign(design, design + (size_t)n_images * n_columns);
    KCHECK(a->d_vals.alloc((size_t)n_images * a->window));
    KCHECK(a->d_design.alloc(a->design.size()));
    KCHECK(hipMemcpy(a->d_design.p, a->design.data(), a->design.size() * sizeof(double), hipMemcpyHostToDevice));
    *out = a.release();
    return FROG_OK;
}

int frog_glm_add(frog_glm *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background)
{
    if (!a || !a->smooth.on) return windowed_add<GlmEntry>("frog_glm_add", a, a ? a->d_vals.p : nullptr, c, src, mask, interpolation, background);
    const SmoothPlan &s = a->smooth;
    if (int rc = windowed_add<GlmEntry>("frog_glm_add", a, a->d_vals.p, c, src, mask, interpolation, background, s.work.d_raw.p, s.first, s.count)) return rc;
    return glm_smooth_store("frog_glm_add", a);
}

int frog_glm_add_jacobian(frog_glm *a, frog_chain *c, const frog_volume *support, const frog_volume *mask, int log_mode)
{
    if (int rc = chain_add_inputs("frog_glm_add_jacobian", a, c, support, mask)) return rc;
    // with smoothing the same kernel on the larger range, into the scratch
    const SmoothPlan &s = a->smooth;
    if (s.on) {
        if (int rc = jacobian_launch("frog_glm_add_jacobian", a, c, support, mask, log_mode, s.first, s.count, s.work.d_raw.p)) return rc;
        return glm_smooth_store("frog_glm_add_jacobian", a);
    }
    if (int rc = jacobian_launch("frog_glm_add_jacobian", a, c, support, mask, log_mode, a->first, a->window, a->d_vals.p + (size_t)a->added * a->window))
        return rc;
    return windowed_added("frog_glm_add_jacobian", a);
}

int frog_glm_plane(frog_glm *a, uint32_t image_index, float *values)
{
    if (!a || !values) return fail(FROG_E_INVALID, "bad arguments to frog_glm_plane");
    if (image_index >= a->added) return fail(FROG_E_INVALID, "frog_glm_plane: that image has not been added");
    KCHECK(hipSetDevice(a->device));
    KCHECK(hipMemcpy(values, a->d_vals.p + (size_t)image_index * a->window, a->window * sizeof(float), hipMemcpyDeviceToHost));
    return FROG_OK;
}

int frog_glm_finish(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                    const uint8_t *region, float fill, float *beta, float *sigma, float *t, uint16_t *count)
{
    if (int rc = glm_fit_arguments("frog_glm_finish", a, n_contrasts, contrasts, min_count, sigma_floor)) return rc;
    if (!t || !n_contrasts) { t = nullptr; n_contrasts = 0; }
    if (!beta && !sigma && !t && !count) return fail(FROG_E_INVALID, "frog_glm_finish: no output asked for");
    KCHECK(hipSetDevice(a->device));
    frog::DevBuf<float> d_beta, d_sigma, d_t;
    frog::DevBuf<uint16_t> d_count;
    frog::DevBuf<uint8_t> d_region;
    if (beta) KCHECK(d_beta.alloc((size_t)a->p * a->window));
    if (sigma) KCHECK(d_sigma.alloc(a->window));
    if (t) KCHECK(d_t.alloc((size_t)n_contrasts * a->window));
    if (count) KCHECK(d_count.alloc(a->window));
    GlmArgs f;
    if (int rc = glm_fit_args("frog_glm_finish", a, n_contrasts, contrasts, min_count, sigma_floor, region, d_region, &f)) return rc;
    f.n_perms = 1;
    f.fill = fill;
    f.beta = d_beta.p;
    f.sigma = d_sigma.p;
    f.t = d_t.p;
    f.count = d_count.p;
    hipError_t e = glm_table_launch(a, nullptr, nullptr, 0, 1);
    if (e == hipSuccess) e = glm_fit_launch(a, f);
    if (e == hipSuccess && beta) e = hipMemcpy(beta, d_beta.p, (size_t)a->p * a->window * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && sigma) e = hipMemcpy(sigma, d_sigma.p, a->window * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && t) e = hipMemcpy(t, d_t.p, (size_t)n_contrasts * a->window * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && count) e = hipMemcpy(count, d_count.p, a->window * sizeof(uint16_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_glm_finish", e);
    return FROG_OK;
}

int frog_glm_permute(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                     const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign,
                     float *max_t, float *min_t)
{
    return glm_permute("frog_glm_permute", a, n_contrasts, contrasts, min_count, sigma_floor, region, columns, n_perms, perm, sign, 0, nullptr, max_t, min_t);
}

int frog_glm_draw(uint32_t n, uint32_t n_perms, uint64_t seed, int shuffle, int flip, uint32_t *perm, int8_t *sign)
{
    if (!perm || (flip && !sign)) return fail(FROG_E_INVALID, "bad arguments to frog_glm_draw");
    if (!n || n > FROG_GLM_MAX_IMAGES || !n_perms) return fail(FROG_E_INVALID, "frog_glm_draw: 1 to " + std::to_string(FROG_GLM_MAX_IMAGES) + " images and at least one permutation");
    uint64_t s = seed;
    auto next = [&s]() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    for (uint32_t k = 0; k < n_perms; k++) {
        uint32_t *row = perm + (size_t)k * n;
        int8_t *sg = sign ? sign + (size_t)k * n : nullptr;
        for (uint32_t i = 0; i < n; i++) row[i] = i;
        if (k && shuffle)
            for (uint32_t i = n - 1; i >= 1; i--) std::swap(row[i], row[next() % (i + 1)]);
        for (uint32_t i = 0; sg && i < n; i++) sg[i] = k && flip && (next() >> 63) ? -1 : 1;
    }
    return FROG_OK;
}

void frog_glm_destroy(frog_glm *a) { group_destroy(a); }

int frog_components(const frog_volume *mask, int connectivity, int device, uint32_t *labels, uint32_t *n_components, uint64_t *largest)
{
    size_t total;
    if (int rc = group_arguments("frog_components", mask, mask, &total)) return rc;
    if (!labels && !n_components && !largest) return fail(FROG_E_INVALID, "frog_components: no output asked for");
    if (!mask->data) return fail(FROG_E_INVALID, "frog_components: a mask without voxels");
    if (!integer_voxel_type(mask->dtype)) return fail(FROG_E_INVALID, "frog_components: a mask has an integer type");
    if (!ccl_order(connectivity)) return fail(FROG_E_INVALID, "frog_components: connectivity 6, 18 or 26");
    const CclGrid g = ccl_grid(mask, total, connectivity);
    std::vector<uint32_t> words(g.words, 0u);
    with_integer_voxel_type(mask->dtype, [&](auto s) { ccl_pack((const decltype(s) *)mask->data, total, words); return FROG_OK; });
    if (int rc = select_device(device)) return rc;
    frog::DevBuf<uint32_t> d_bits, d_parent, d_extent, d_stats;
    KCHECK(d_bits.alloc(g.words));
    KCHECK(d_parent.alloc(total));
    KCHECK(d_extent.alloc(total));
    KCHECK(d_stats.alloc(2));
    uint32_t stats[2] = { 0, 0 }, n = 0;
    hipError_t e = hipMemcpy(d_bits.p, words.data(), g.words * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_stats.p, 0, sizeof stats);
    if (e == hipSuccess) e = ccl_label(g, d_bits.p, 1, d_parent.p, d_extent.p, d_stats.p);
    if (e == hipSuccess) e = hipMemcpy(stats, d_stats.p, sizeof stats, hipMemcpyDeviceToHost);
    if (e == hipSuccess && labels) e = ccl_labels_out(g, d_bits.p, d_parent.p, labels, &n);
    if (e != hipSuccess) return hip_fail("frog_components", e);
    if (n_components) *n_components = stats[0];
    if (largest) *largest = stats[1];
    return FROG_OK;
}

int frog_clusters_create(const frog_volume *grid, uint32_t n_perms, uint32_t n_contrasts, int two_sided, float threshold, int connectivity,
                         int device, frog_clusters **out)
{
    std::unique_ptr<frog_clusters> s;
    // a slot keeps its mask and two words of statistics; a slot's workspace is two words per voxel
    if (int rc = sink_new("frog_clusters_create", "masks", grid, n_perms, n_contrasts, two_sided, connectivity, device, out, [&]() {
            const bool good = threshold >= 0.0f && std::isfinite(threshold);
            return good ? (int)FROG_OK : fail(FROG_E_INVALID, "frog_clusters_create: the threshold must be finite and not negative");
        }, [](const CclGrid &g) { return std::make_pair(g.words * sizeof(uint32_t) + 2 * sizeof(uint32_t), g.total * 2 * sizeof(uint32_t)); }, s)) return rc;
    KCHECK(s->d_bits.alloc(s->slots * s->ccl.words));
    KCHECK(s->d_stats.alloc(s->slots * 2));
    KCHECK(s->d_parent.alloc((size_t)s->batch * s->total));
    KCHECK(s->d_extent.alloc((size_t)s->batch * s->total));
    KCHECK(hipMemset(s->d_bits.p, 0, s->d_bits.bytes()));
    s->store.kind = GlmStore::BITS;
    s->store.bits = GlmSink{ s->d_bits.p, s->ccl.words, 0, 0, s->sides, threshold };
    *out = s.release();
    return FROG_OK;
}

int frog_glm_permute_clusters(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                              const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign,
                              uint32_t first_perm, frog_clusters *sink, float *max_t, float *min_t)
{
    if (!sink) return fail(FROG_E_INVALID, "bad arguments to frog_glm_permute_clusters");
    return glm_permute("frog_glm_permute_clusters", a, n_contrasts, contrasts, min_count, sigma_floor, region, columns, n_perms, perm, sign, first_perm, sink, max_t, min_t);
}

int frog_clusters_finish(frog_clusters *s, uint32_t *max_extent)
{
    std::vector<uint32_t> stats(s ? s->slots * 2 : 0);
    if (int rc = sink_finish("frog_clusters_finish", s, max_extent, [&](size_t at, uint32_t n) {
            const hipError_t e = hipMemset(s->d_stats.p + 2 * at, 0, 2 * n * sizeof(uint32_t));
            return e != hipSuccess ? e : ccl_label(s->ccl, s->d_bits.p + at * s->ccl.words, n, s->d_parent.p, s->d_extent.p, s->d_stats.p + 2 * at);
        }, [&]() { return hipMemcpy(stats.data(), s->d_stats.p, s->d_stats.bytes(), hipMemcpyDeviceToHost); })) return rc;
    for (size_t k = 0; k < s->slots; k++) max_extent[k] = stats[2 * k + 1];
    return FROG_OK;
}

int frog_clusters_mask(frog_clusters *s, uint32_t perm, uint32_t contrast, int side, uint8_t *mask)
{
    size_t slot;
    if (int rc = sink_slot("frog_clusters_mask", s, perm, contrast, side, mask, false, &slot)) return rc;
    frog::DevBuf<uint8_t> d_out;
    KCHECK(d_out.alloc(s->total));
    const uint32_t *d_mask = s->d_bits.p + slot * s->ccl.words;
    hipError_t e = chunked_launch(s->total, [&](unsigned blocks, size_t base) {
        ccl_bytes_kernel<<<blocks, LAUNCH_BLOCK>>>(base, d_mask, s->total, d_out.p);
    });
    if (e == hipSuccess) e = hipMemcpy(mask, d_out.p, s->total, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_clusters_mask", e);
    return FROG_OK;
}

int frog_clusters_labels(frog_clusters *s, uint32_t perm, uint32_t contrast, int side, uint32_t *labels, uint32_t *n_components)
{
    size_t slot;
    if (int rc = sink_slot("frog_clusters_labels", s, perm, contrast, side, labels, true, &slot)) return rc;
    const uint32_t *d_mask = s->d_bits.p + slot * s->ccl.words;
    uint32_t n = 0;
    hipError_t e = ccl_label(s->ccl, d_mask, 1, s->d_parent.p, s->d_extent.p, nullptr);
    if (e == hipSuccess) e = ccl_labels_out(s->ccl, d_mask, s->d_parent.p, labels, &n);
    if (e != hipSuccess) return hip_fail("frog_clusters_labels", e);
    if (n_components) *n_components = n;
    return FROG_OK;
}

void frog_clusters_destroy(frog_clusters *s) { group_destroy(s); }

int frog_tfce_create(const frog_volume *grid, uint32_t n_perms, uint32_t n_contrasts, int two_sided, float dh, double E, double H,
                     int connectivity, int device, frog_tfce **out)
{
    TfceParams par;
    std::unique_ptr<frog_tfce> s;
    // a slot keeps its levels, its highest level and its largest tfce
    if (int rc = sink_new("frog_tfce_create", "level maps", grid, n_perms, n_contrasts, two_sided, connectivity, device, out,
                          [&]() { return tfce_params("frog_tfce_create", dh, E, H, connectivity, &par); },
                          [](const CclGrid &g) { return std::make_pair(tfce_stride(g) + 2 * sizeof(uint32_t), tfce_work_bytes(g)); }, s)) return rc;
    s->par = par;
    s->stride = tfce_stride(s->ccl);
    KCHECK(s->d_levels.alloc(s->slots * s->stride));
    KCHECK(s->d_top.alloc(s->slots));
    KCHECK(s->d_best.alloc(s->slots));
    KCHECK(tfce_work_alloc(s->work, s->ccl, s->batch));
    KCHECK(hipMemset(s->d_levels.p, 0, s->d_levels.bytes()));
    s->store.kind = GlmStore::LEVELS;
    s->store.levels = GlmLevelSink{ s->d_levels.p, s->stride, 0, 0, s->sides, par.dh };
    *out = s.release();
    return FROG_OK;
}

int frog_glm_permute_tfce(frog_glm *a, uint32_t n_contrasts, const double *contrasts, uint32_t min_count, double sigma_floor,
                          const uint8_t *region, uint32_t columns, uint32_t n_perms, const uint32_t *perm, const int8_t *sign,
                          uint32_t first_perm, frog_tfce *sink, float *max_t, float *min_t)
{
    if (!sink) return fail(FROG_E_INVALID, "bad arguments to frog_glm_permute_tfce");
    return glm_permute("frog_glm_permute_tfce", a, n_contrasts, contrasts, min_count, sigma_floor, region, columns, n_perms, perm, sign, first_perm, sink, max_t, min_t);
}

int frog_tfce_finish(frog_tfce *s, float *max_tfce)
{
    return sink_finish("frog_tfce_finish", s, max_tfce, [&](size_t at, uint32_t n) {
        return tfce_enhance(s->ccl, s->par, s->d_levels.p + at * s->stride, s->stride, n, s->work, s->d_top.p + at, nullptr, s->d_best.p + at);
    }, [&]() { return hipMemcpy(max_tfce, s->d_best.p, s->slots * sizeof(float), hipMemcpyDeviceToHost); });   // the bits of f32 values
}

int frog_tfce_levels(frog_tfce *s, uint32_t perm, uint32_t contrast, int side, uint8_t *levels)
{
    size_t slot;
    if (int rc = sink_slot("frog_tfce_levels", s, perm, contrast, side, levels, false, &slot)) return rc;
    KCHECK(hipMemcpy(levels, s->d_levels.p + slot * s->stride, s->total, hipMemcpyDeviceToHost));
    return FROG_OK;
}

int frog_tfce_map(frog_tfce *s, uint32_t perm, uint32_t contrast, int side, float *tfce)
{
    size_t slot;
    if (int rc = sink_slot("frog_tfce_map", s, perm, contrast, side, tfce, true, &slot)) return rc;
    frog::DevBuf<float> d_map;
    KCHECK(d_map.alloc(s->total));
    hipError_t e = tfce_enhance(s->ccl, s->par, s->d_levels.p + slot * s->stride, s->stride, 1, s->work, s->d_top.p + slot, d_map.p, s->d_best.p + slot);
    if (e == hipSuccess) e = hipMemcpy(tfce, d_map.p, s->total * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_tfce_map", e);
    return FROG_OK;
}

void frog_tfce_destroy(frog_tfce *s) { group_destroy(s); }

int frog_tfce_volume(const frog_volume *stat, int side, float dh, double E, double H, int connectivity, int device, float *tfce, float *max)
{
    size_t total;
    if (int rc = group_arguments("frog_tfce_volume", stat, stat, &total)) return rc;
    if (!tfce && !max) return fail(FROG_E_INVALID, "frog_tfce_volume: no output asked for");
    if (!stat->data) return fail(FROG_E_INVALID, "frog_tfce_volume: a volume without voxels");
    if (stat->dtype != FROG_V_F32) return fail(FROG_E_INVALID, "frog_tfce_volume: the volume has type FROG_V_F32");
    if (side != 0 && side != 1) return fail(FROG_E_INVALID, "frog_tfce_volume: side 0 or 1");
    TfceParams par;
    if (int rc = tfce_params("frog_tfce_volume", dh, E, H, connectivity, &par)) return rc;
    const CclGrid g = ccl_grid(stat, total, connectivity);
    if (int rc = select_device(device)) return rc;
    frog::DevBuf<float> d_stat, d_map;
    frog::DevBuf<uint8_t> d_levels;
    frog::DevBuf<uint32_t> d_slot;                  // the highest level, the bits of the largest tfce
    TfceWork work;
    KCHECK(d_stat.alloc(total));
    KCHECK(d_map.alloc(total));
    KCHECK(d_levels.alloc(tfce_stride(g)));
    KCHECK(d_slot.alloc(2));
    KCHECK(tfce_work_alloc(work, g, 1));
    hipError_t e = hipMemcpy(d_stat.p, stat->data, total * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_levels.p, 0, d_levels.bytes());
    if (e == hipSuccess) e = chunked_launch(total, [&](unsigned blocks, size_t base) {
        tfce_levels_kernel<<<blocks, LAUNCH_BLOCK>>>(base, d_stat.p, total, (uint32_t)side, dh, d_levels.p);
    });
    if (e == hipSuccess) e = tfce_enhance(g, par, d_levels.p, tfce_stride(g), 1, work, d_slot.p, d_map.p, d_slot.p + 1);
    if (e == hipSuccess && tfce) e = hipMemcpy(tfce, d_map.p, total * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && max) e = hipMemcpy(max, d_slot.p + 1, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_tfce_volume", e);
    return FROG_OK;
}

int frog_smooth_taps(double sigma_mm, double spacing, uint32_t *radius, double *taps)
{
    if (!radius) return fail(FROG_E_INVALID, "bad arguments to frog_smooth_taps");
    if (!(sigma_mm > 0.0) || !std::isfinite(sigma_mm)) return fail(FROG_E_INVALID, "frog_smooth_taps: sigma is finite and above 0");
    if (!(spacing > 0.0) || !std::isfinite(spacing)) return fail(FROG_E_INVALID, "frog_smooth_taps: the spacing is finite and above 0");
    volatile double q = 3.0 * sigma_mm;             // volatile: every line is rounded to f64 on its own, whatever the host compiler contracts
    q = q / spacing;
    const double r = std::ceil(q);
    if (!(r <= (double)FROG_SMOOTH_MAX_RADIUS))
        return fail(FROG_E_INVALID, "frog_smooth_taps: a radius of " + std::to_string(r) + " voxels, above " + std::to_string(FROG_SMOOTH_MAX_RADIUS));
    *radius = (uint32_t)r;
    if (!taps) return FROG_OK;
    volatile double den = 2.0 * sigma_mm;
    den = den * sigma_mm;
    for (uint32_t d = 0; d <= *radius; d++) {
        volatile double x = (double)d * spacing;
        x = x * x;
        x = x / den;
        taps[d] = std::exp(-x);
    }
    return FROG_OK;
}

int frog_smooth_volume(const frog_volume *volume, const uint8_t *take, double sigma_mm, int device, float *out)
{
    size_t total;
    if (int rc = group_arguments("frog_smooth_volume", volume, out, &total)) return rc;
    if (!volume->data) return fail(FROG_E_INVALID, "frog_smooth_volume: a volume without voxels");
    if (volume->dtype != FROG_V_F32) return fail(FROG_E_INVALID, "frog_smooth_volume: the volume has type FROG_V_F32");
    SmoothWork work;
    if (int rc = smooth_taps3("frog_smooth_volume", volume, sigma_mm, work.taps)) return rc;
    if (int rc = select_device(device)) return rc;
    frog::DevBuf<uint8_t> d_take;
    frog::DevBuf<float> d_out;
    KCHECK(smooth_work_alloc(work, total));
    KCHECK(d_out.alloc(total));
    if (take) KCHECK(d_take.alloc(total));
    hipError_t e = hipMemcpy(work.d_raw.p, volume->data, total * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && take) e = hipMemcpy(d_take.p, take, total, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = smooth_passes(*volume, work, d_take.p, total, 0, total, d_out.p);
    if (e == hipSuccess) e = hipMemcpy(out, d_out.p, total * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_smooth_volume", e);
    return FROG_OK;
}

int frog_glm_smooth(frog_glm *a, double sigma_mm)
{
    if (!a) return fail(FROG_E_INVALID, "bad arguments to frog_glm_smooth");
    SmoothTaps taps[3];
    if (int rc = smooth_taps3("frog_glm_smooth", &a->grid, sigma_mm, taps)) return rc;
    if (a->added) return fail(FROG_E_STATE, "frog_glm_smooth: after the first add");
    KCHECK(hipSetDevice(a->device));
    SmoothPlan &s = a->smooth;
    s.on = false;
    s.work.d_raw.release();
    s.work.d_x.release();
    s.work.d_y.release();
    if (sigma_mm == 0.0) return FROG_OK;
    const size_t plane = (size_t)a->grid.dims[0] * a->grid.dims[1];
    uint32_t first, count;
    smooth_range(a->grid.dims[2], (uint32_t)(a->first / plane), (uint32_t)(a->window / plane), taps[2].radius, &first, &count);
    const size_t voxels = plane * count, need = voxels * SMOOTH_VOXEL_BYTES;
    size_t free_bytes = 0;
    KCHECK(smooth_free_bytes(&free_bytes));
    if (need > free_bytes)
        return fail(FROG_E_NOMEM, "frog_glm_smooth: the scratch of " + std::to_string(count) + " planes needs " + std::to_string(need) +
                                      " bytes of device memory, " + std::to_string(free_bytes) + " are free");
    KCHECK(smooth_work_alloc(s.work, voxels));
    for (int k = 0; k < 3; k++) s.work.taps[k] = taps[k];
    s.first = plane * first;
    s.count = voxels;
    s.on = true;
    return FROG_OK;
}

int frog_glm_smooth_planes(const frog_volume *grid, uint32_t n_images, double sigma_mm, int device, uint32_t *planes)
{
    if (!grid || !planes) return fail(FROG_E_INVALID, "bad arguments to frog_glm_smooth_planes");
    SmoothTaps taps[3];
    if (int rc = smooth_taps3("frog_glm_smooth_planes", grid, sigma_mm, taps)) return rc;
    uint32_t fit = 0;
    if (int rc = frog_glm_planes(grid, n_images, device, &fit)) return rc;
    if (sigma_mm == 0.0) { *planes = fit; return FROG_OK; }
    size_t free_bytes = 0;
    KCHECK(smooth_free_bytes(&free_bytes));
    const size_t plane = (size_t)grid->dims[0] * grid->dims[1], depth = grid->dims[2], halo = 2 * (size_t)taps[2].radius;
    auto bytes = [&](size_t p) { return plane * (p * sizeof(float) * n_images + std::min(p + halo, depth) * SMOOTH_VOXEL_BYTES); };
    // bytes() grows with p: the largest p that fits, by bisection
    size_t lo = 0, hi = fit;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (bytes(mid) <= free_bytes / 2) lo = mid; else hi = mid - 1;
    }
    if (!lo) return fail(FROG_E_INVALID, "frog_glm_smooth_planes: not one plane of the grid and the scratch of its halo fit half of the free device memory");
    *planes = (uint32_t)lo;
    return FROG_OK;
}

int frog_labels_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, int device, frog_labels **out)
{
    size_t total;
    if (int rc = group_arguments("frog_labels_create", grid, out, &total)) return rc;
    if (!n_images || n_images > 65535) return fail(FROG_E_INVALID, "frog_labels_create: 1 to 65535 images (16-bit vote counts)");
    if (max_labels > 65536) return fail(FROG_E_INVALID, "frog_labels_create: max_labels above 65536");
    std::unique_ptr<frog_labels> a;
    if (int rc = group_new(grid, total, device, a)) return rc;
    a->n_images = n_images;
    if (int rc = labels_new_map(a.get(), max_labels ? max_labels : 1024)) return rc;
    KCHECK(a->d_planes.alloc(a->max_labels));
    *out = a.release();
    return FROG_OK;
}

int frog_labels_add(frog_labels *a, frog_chain *c, const frog_volume *src, double background, frog_volume *resliced)
{
    if (!a || !src || !src->data) return fail(FROG_E_INVALID, "bad arguments to frog_labels_add");
    if (!integer_voxel_type(src->dtype)) return fail(FROG_E_INVALID, "frog_labels_add: a label volume has an integer type");
    if (!std::isfinite(background)) return fail(FROG_E_INVALID, "frog_labels_add: background is not finite");
    if (a->finished || a->added >= a->n_images) return fail(FROG_E_INVALID, "frog_labels_add: more volumes than n_images");
    if (int rc = add_inputs("frog_labels_add", a, c, src, resliced)) return rc;
    KCHECK(hipSetDevice(a->device));
    const int rc = with_integer_voxel_type(src->dtype, [&](auto s) { return labels_add_typed<decltype(s)>(a, c, src, background, resliced); });
    if (rc == FROG_OK) a->added++;
    return rc;
}

int frog_labels_finish(frog_labels *a, uint32_t *n_labels)
{
    if (!a || !n_labels) return fail(FROG_E_INVALID, "bad arguments to frog_labels_finish");
    if (a->added != a->n_images) return fail(FROG_E_INVALID, "frog_labels_finish: fewer volumes added than n_images");
    if (a->finished) { *n_labels = (uint32_t)a->values.size(); return FROG_OK; }
    KCHECK(hipSetDevice(a->device));
    const size_t n_planes = a->known.size();
    std::vector<unsigned long long> sums(LABEL_SUM_STRIDE * n_planes, 0);
    frog::DevBuf<unsigned long long> d_sums;
    KCHECK(d_sums.alloc(sums.size()));
    KCHECK(hipMemset(d_sums.p, 0, sums.size() * sizeof(unsigned long long)));
    const size_t tile = (size_t)LABEL_TABLE_ITEMS * LAUNCH_BLOCK, blocks_per_plane = (a->total + tile - 1) / tile;
    hipError_t e = chunked_launch(n_planes * blocks_per_plane * LAUNCH_BLOCK, [&](unsigned blocks, size_t base) {
        labels_table_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_planes.p, (uint32_t)n_planes, a->total, blocks_per_plane, d_sums.p);
    });
    if (e == hipSuccess) e = hipMemcpy(sums.data(), d_sums.p, sums.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_labels_finish", e);
    std::vector<uint32_t> order;                    // the labels without a vote do not enter the table
    for (size_t i = 0; i < n_planes; i++) if (sums[LABEL_SUM_STRIDE * i]) order.push_back((uint32_t)i);
    if (int rc = labels_sort(a, order)) return rc;
    if (int rc = labels_sort_planes(order, a->planes, a->d_sorted_planes)) return rc;
    a->voxels.clear(); a->pairs.clear();
    for (const uint32_t i : order) {
        a->voxels.push_back(sums[LABEL_SUM_STRIDE * i]);
        a->pairs.push_back(sums[LABEL_SUM_STRIDE * i + 1]);
    }
    a->dense = order;
    a->finished = true;
    *n_labels = (uint32_t)order.size();
    return FROG_OK;
}

int frog_labels_table(frog_labels *a, int64_t *values, uint64_t *voxels, uint64_t *pairs)
{
    if (!a || !values || !voxels || !pairs) return fail(FROG_E_INVALID, "bad arguments to frog_labels_table");
    if (!a->finished) return fail(FROG_E_INVALID, "frog_labels_table: before frog_labels_finish");
    for (size_t l = 0; l < a->values.size(); l++) { values[l] = a->values[l]; voxels[l] = a->voxels[l]; pairs[l] = a->pairs[l]; }
    return FROG_OK;
}

int frog_labels_fused(frog_labels *a, frog_volume *label, float *agreement)
{
    if (int rc = fused_arguments("frog_labels_fused", a, a && a->finished, "frog_labels_finish", label, agreement)) return rc;
    return with_integer_voxel_type(label ? label->dtype : FROG_V_I32, [&](auto t) {
        using T = decltype(t);
        if (label && !labels_fit<T>(a)) return fail(FROG_E_INVALID, "frog_labels_fused: a label value does not fit the requested type");
        return fused_output<T>("frog_labels_fused", a, label, agreement, [&](unsigned blocks, size_t base, T *d_label, float *d_agreement) {
            labels_fused_kernel<T><<<blocks, LAUNCH_BLOCK>>>(base, a->d_sorted_planes.p, a->d_sorted_values.p, (uint32_t)a->values.size(), a->total,
                                                             (float)a->n_images, d_label, d_agreement);
        });
    });
}

int frog_labels_probability(frog_labels *a, int64_t value, float *p)
{
    size_t l;
    if (int rc = labels_getter("frog_labels_probability", a && p, a && a->finished, "frog_labels_finish")) return rc;
    if (int rc = labels_find("frog_labels_probability", "no such label in the table", a, value, &l)) return rc;
    const uint16_t *plane = a->planes[a->dense[l]].p;
    return probability_output("frog_labels_probability", a, p, [&](unsigned blocks, size_t base, float *d_p) {
        labels_probability_kernel<<<blocks, LAUNCH_BLOCK>>>(base, plane, a->total, (float)a->n_images, d_p);
    });
}

void frog_labels_destroy(frog_labels *a) { group_destroy(a); }

int frog_staple_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, int device, frog_staple **out)
{
    size_t total;
    if (int rc = group_arguments("frog_staple_create", grid, out, &total)) return rc;
    if (!n_images || n_images > 4096) return fail(FROG_E_INVALID, "frog_staple_create: 1 to 4096 images");
    if (max_labels > FROG_STAPLE_MAX_LABELS) return fail(FROG_E_INVALID, "frog_staple_create: max_labels above 256 (one byte per image and voxel)");
    std::unique_ptr<frog_staple> a;
    if (int rc = group_new(grid, total, device, a)) return rc;
    a->n_images = n_images;
    KCHECK(a->d_D.alloc((size_t)n_images * total));
    if (int rc = labels_new_map(a.get(), max_labels ? max_labels : FROG_STAPLE_MAX_LABELS)) return rc;
    *out = a.release();
    return FROG_OK;
}

int frog_staple_add(frog_staple *a, frog_chain *c, const frog_volume *src, double background, frog_volume *resliced)
{
    if (!a || !src || !src->data) return fail(FROG_E_INVALID, "bad arguments to frog_staple_add");
    if (!integer_voxel_type(src->dtype)) return fail(FROG_E_INVALID, "frog_staple_add: a label volume has an integer type");
    if (!std::isfinite(background)) return fail(FROG_E_INVALID, "frog_staple_add: background is not finite");
    if (a->finished || a->added >= a->n_images) return fail(FROG_E_INVALID, "frog_staple_add: more volumes than n_images");
    if (int rc = add_inputs("frog_staple_add", a, c, src, resliced)) return rc;
    KCHECK(hipSetDevice(a->device));
    const int rc = with_integer_voxel_type(src->dtype, [&](auto s) { return staple_add_typed<decltype(s)>(a, c, src, background, resliced); });
    if (rc == FROG_OK) a->added++;
    return rc;
}

int frog_staple_finish(frog_staple *a, uint32_t *n_labels)
{
    if (!a || !n_labels) return fail(FROG_E_INVALID, "bad arguments to frog_staple_finish");
    if (a->added != a->n_images) return fail(FROG_E_INVALID, "frog_staple_finish: fewer volumes added than n_images");
    if (a->finished) { *n_labels = (uint32_t)a->values.size(); return FROG_OK; }
    KCHECK(hipSetDevice(a->device));
    const size_t L = a->known.size(), entries = (size_t)a->n_images * L * L;
    std::vector<uint32_t> order = labels_all(a);
    if (int rc = labels_sort(a, order)) return rc;
    StapleLut lut{};
    for (size_t l = 0; l < L; l++) lut.to[order[l]] = (uint8_t)l;
    KCHECK(a->d_active.alloc(a->total));
    KCHECK(a->d_q.alloc(L * a->total));
    KCHECK(a->d_theta.alloc(entries));
    KCHECK(a->d_S.alloc(entries));
    KCHECK(a->d_T.alloc(L));
    KCHECK(a->d_prior.alloc(L));
    KCHECK(a->d_word.alloc(L + 1));
    const size_t count = (size_t)a->n_images * a->total;
    KCHECK(chunked_launch(count, [&](unsigned blocks, size_t base) {
        staple_renumber_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_D.p, count, lut);
    }));
    KCHECK(hipStreamSynchronize(0));
    a->finished = true;
    *n_labels = (uint32_t)L;
    return FROG_OK;
}

int frog_staple_values(frog_staple *a, int64_t *values) { return labels_values("frog_staple_values", a, "frog_staple_finish", values); }

int frog_staple_solve(frog_staple *a, double p0, double tol, uint32_t max_iter, int restrict_to_disputed,
                      uint32_t *iterations, double *change, uint64_t *active_voxels)
{
    if (!a || !iterations || !change || !active_voxels) return fail(FROG_E_INVALID, "bad arguments to frog_staple_solve");
    if (!(p0 > 0.0 && p0 < 1.0)) return fail(FROG_E_INVALID, "frog_staple_solve: p0 inside (0, 1)");
    if (!(tol >= 0.0)) return fail(FROG_E_INVALID, "frog_staple_solve: a tolerance that is not negative");
    if (!a->finished) return fail(FROG_E_INVALID, "frog_staple_solve: before frog_staple_finish");
    KCHECK(hipSetDevice(a->device));
    const uint32_t n = a->n_images, L = (uint32_t)a->values.size();
    const size_t entries = (size_t)n * L * L;
    a->solved = false;
    std::vector<unsigned long long> c(L);
    KCHECK(hipMemset(a->d_word.p, 0, L * sizeof(unsigned long long)));
    KCHECK(chunked_launch(a->total, [&](unsigned blocks, size_t base) {
        staple_active_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_D.p, a->total, n, L, restrict_to_disputed != 0, a->d_active.p, a->d_q.p, a->d_word.p);
    }));
    KCHECK(hipMemcpy(c.data(), a->d_word.p, L * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long entries_active = 0;
    for (const unsigned long long x : c) entries_active += x;
    const unsigned long long A = entries_active / n;
    a->prior.assign(L, 0.0);
    a->theta.assign(entries, 0.0);
    a->sums.assign(entries, 0);
    a->totals.assign(L, 0);
    const double off = L > 1 ? (1.0 - p0) / (double)(L - 1) : 0.0;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t lp = 0; lp < L; lp++)
            for (uint32_t l = 0; l < L; l++) a->theta[((size_t)i * L + lp) * L + l] = lp == l ? p0 : off;
    uint32_t it = 0;
    double ch = INFINITY;
    if (A) {
        for (uint32_t l = 0; l < L; l++) a->prior[l] = (double)c[l] / (double)((unsigned long long)n * A);
        KCHECK(hipMemcpy(a->d_prior.p, a->prior.data(), L * sizeof(double), hipMemcpyHostToDevice));
        KCHECK(hipMemcpy(a->d_theta.p, a->theta.data(), entries * sizeof(double), hipMemcpyHostToDevice));
        for (;;) {
            KCHECK(staple_estep_launch(a));
            if (it == max_iter) break;
            if (int rc = staple_mstep(a, &ch)) return rc;
            it++;
            if (ch < tol) { KCHECK(staple_estep_launch(a)); break; }
        }
        KCHECK(hipMemcpy(a->theta.data(), a->d_theta.p, entries * sizeof(double), hipMemcpyDeviceToHost));
        if (it) {
            KCHECK(hipMemcpy(a->sums.data(), a->d_S.p, entries * sizeof(uint64_t), hipMemcpyDeviceToHost));
            KCHECK(hipMemcpy(a->totals.data(), a->d_T.p, L * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
    }
    KCHECK(hipStreamSynchronize(0));
    a->solved = true;
    *iterations = it;
    *change = ch;
    *active_voxels = A;
    return FROG_OK;
}

int frog_staple_fused(frog_staple *a, frog_volume *label, float *confidence)
{
    if (int rc = fused_arguments("frog_staple_fused", a, a && a->solved, "frog_staple_solve", label, confidence)) return rc;
    return with_integer_voxel_type(label ? label->dtype : FROG_V_I32, [&](auto t) {
        using T = decltype(t);
        if (label && !labels_fit<T>(a)) return fail(FROG_E_INVALID, "frog_staple_fused: a label value does not fit the requested type");
        return fused_output<T>("frog_staple_fused", a, label, confidence, [&](unsigned blocks, size_t base, T *d_label, float *d_confidence) {
            staple_fused_kernel<T><<<blocks, LAUNCH_BLOCK>>>(base, a->d_q.p, a->d_sorted_values.p, (uint32_t)a->values.size(), a->total,
                                                             d_label, d_confidence);
        });
    });
}

int frog_staple_probability(frog_staple *a, int64_t value, float *p)
{
    size_t l;
    if (int rc = labels_getter("frog_staple_probability", a && p, a && a->solved, "frog_staple_solve")) return rc;
    if (int rc = labels_find("frog_staple_probability", "no such label", a, value, &l)) return rc;
    const uint32_t *plane = a->d_q.p + l * a->total;
    return probability_output("frog_staple_probability", a, p, [&](unsigned blocks, size_t base, float *d_p) {
        staple_probability_kernel<<<blocks, LAUNCH_BLOCK>>>(base, plane, a->total, d_p);
    });
}

int frog_staple_performance(frog_staple *a, double *theta, uint64_t *sums, uint64_t *totals, double *prior)
{
    if (!a || (!theta && !sums && !totals && !prior)) return fail(FROG_E_INVALID, "bad arguments to frog_staple_performance");
    if (!a->solved) return fail(FROG_E_INVALID, "frog_staple_performance: before frog_staple_solve");
    if (theta) std::copy(a->theta.begin(), a->theta.end(), theta);
    if (sums) std::copy(a->sums.begin(), a->sums.end(), sums);
    if (totals) std::copy(a->totals.begin(), a->totals.end(), totals);
    if (prior) std::copy(a->prior.begin(), a->prior.end(), prior);
    return FROG_OK;
}

void frog_staple_destroy(frog_staple *a) { group_destroy(a); }

int frog_wlabels_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, uint32_t radius, uint32_t power, float floor,
                        int device, frog_wlabels **out)
{
    size_t total;
    if (int rc = group_arguments("frog_wlabels_create", grid, out, &total)) return rc;
    if (!n_images) return fail(FROG_E_INVALID, "frog_wlabels_create: at least one image");
    if (max_labels > 65536) return fail(FROG_E_INVALID, "frog_wlabels_create: max_labels above 65536");
    if (radius < 1 || radius > 4) return fail(FROG_E_INVALID, "frog_wlabels_create: a radius from 1 to 4");
    if (power < 1 || power > 8) return fail(FROG_E_INVALID, "frog_wlabels_create: a power from 1 to 8");
    if (!(floor >= 0.0f && floor <= 1.0f)) return fail(FROG_E_INVALID, "frog_wlabels_create: a floor in [0, 1]");
    std::unique_ptr<frog_wlabels> a;
    if (int rc = group_new(grid, total, device, a)) return rc;
    a->n_images = n_images;
    a->radius = radius;
    a->power = power;
    a->floor = floor;
    KCHECK(a->d_target.alloc(total));
    KCHECK(a->d_atlas.alloc(total));
    if (int rc = labels_new_map(a.get(), max_labels ? max_labels : 1024)) return rc;
    KCHECK(a->d_planes.alloc(a->max_labels));
    *out = a.release();
    return FROG_OK;
}

// frog_wlabels_target and frog_jlabels_target under their names
static int wlabels_target(const char *where, frog_wlabels *a, frog_chain *c, const frog_volume *src, int interpolation, double background,
                          frog_volume *resliced)
{
    if (!a || !src || !src->data || !frog_volume_voxel_bytes(src->dtype)) return fail(FROG_E_INVALID, std::string("bad arguments to ") + where);
    if (a->has_target) return fail(FROG_E_INVALID, std::string(where) + ": the target is given once, before the first add");
    if (int rc = add_inputs(where, a, c, src, resliced)) return rc;
    KCHECK(hipSetDevice(a->device));
    const int rc = with_voxel_type(src->dtype, [&](auto s) { return wlabels_target_typed<decltype(s)>(where, a, c, src, interpolation, background, resliced); });
    if (rc == FROG_OK) a->has_target = true;
    return rc;
}

int frog_wlabels_target(frog_wlabels *a, frog_chain *c, const frog_volume *src, int interpolation, double background, frog_volume *resliced)
{
    return wlabels_target("frog_wlabels_target", a, c, src, interpolation, background, resliced);
}

int frog_wlabels_add(frog_wlabels *a, frog_chain *c, const frog_volume *image, const frog_volume *labels, int interpolation,
                     double image_background, double label_background, frog_volume *resliced_image, frog_volume *resliced_labels)
{
    if (!a || !image || !image->data || !frog_volume_voxel_bytes(image->dtype) || !labels || !labels->data)
        return fail(FROG_E_INVALID, "bad arguments to frog_wlabels_add");
    if (!integer_voxel_type(labels->dtype)) return fail(FROG_E_INVALID, "frog_wlabels_add: a label volume has an integer type");
    if (!std::isfinite(image_background) || !std::isfinite(label_background)) return fail(FROG_E_INVALID, "frog_wlabels_add: background is not finite");
    if (!a->has_target) return fail(FROG_E_INVALID, "frog_wlabels_add: before frog_wlabels_target");
    if (a->finished || a->added >= a->n_images) return fail(FROG_E_INVALID, "frog_wlabels_add: more atlases than n_images");
    if (int rc = add_inputs("frog_wlabels_add", a, c, image, resliced_image)) return rc;
    if (int rc = add_inputs("frog_wlabels_add", a, c, labels, resliced_labels)) return rc;
    KCHECK(hipSetDevice(a->device));
    const int rc = with_voxel_type(image->dtype, [&](auto s) {
        return wlabels_add_typed<decltype(s)>(a, c, image, labels, interpolation, image_background, label_background, resliced_image, resliced_labels);
    });
    if (rc == FROG_OK) a->added++;
    return rc;
}

int frog_wlabels_finish(frog_wlabels *a, uint32_t *n_labels)
{
    if (!a || !n_labels) return fail(FROG_E_INVALID, "bad arguments to frog_wlabels_finish");
    if (a->added != a->n_images) return fail(FROG_E_INVALID, "frog_wlabels_finish: fewer atlases added than n_images");
    if (a->finished) { *n_labels = (uint32_t)a->values.size(); return FROG_OK; }
    KCHECK(hipSetDevice(a->device));
    std::vector<uint32_t> order = labels_all(a);
    if (int rc = labels_sort(a, order)) return rc;
    if (int rc = labels_sort_planes(order, a->planes, a->d_sorted_planes)) return rc;
    a->dense = order;
    a->finished = true;
    *n_labels = (uint32_t)order.size();
    return FROG_OK;
}

int frog_wlabels_values(frog_wlabels *a, int64_t *values) { return labels_values("frog_wlabels_values", a, "frog_wlabels_finish", values); }

int frog_wlabels_fused(frog_wlabels *a, int64_t fill_label, frog_volume *label, float *confidence)
{
    if (int rc = fused_arguments("frog_wlabels_fused", a, a && a->finished, "frog_wlabels_finish", label, confidence)) return rc;
    const long long fill = label ? (long long)fill_label : 0;
    return with_integer_voxel_type(label ? label->dtype : FROG_V_I32, [&](auto t) {
        using T = decltype(t);
        if (label && (!labels_fit<T>(a) || fill < (long long)std::numeric_limits<T>::lowest() || fill > (long long)std::numeric_limits<T>::max()))
            return fail(FROG_E_INVALID, "frog_wlabels_fused: a label value or the fill label does not fit the requested type");
        return fused_output<T>("frog_wlabels_fused", a, label, confidence, [&](unsigned blocks, size_t base, T *d_label, float *d_confidence) {
            wlabels_fused_kernel<T><<<blocks, LAUNCH_BLOCK>>>(base, a->d_sorted_planes.p, a->d_sorted_values.p, (uint32_t)a->values.size(), a->total,
                                                              (T)fill, d_label, d_confidence);
        });
    });
}

int frog_wlabels_probability(frog_wlabels *a, int64_t value, float *p)
{
    size_t l;
    if (int rc = labels_getter("frog_wlabels_probability", a && p, a && a->finished, "frog_wlabels_finish")) return rc;
    if (int rc = labels_find("frog_wlabels_probability", "no such label in the table", a, value, &l)) return rc;
    return probability_output("frog_wlabels_probability", a, p, [&](unsigned blocks, size_t base, float *d_p) {
        wlabels_probability_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_sorted_planes.p, (uint32_t)a->values.size(), (uint32_t)l, a->total, d_p);
    });
}

void frog_wlabels_destroy(frog_wlabels *a) { group_destroy(a); }

int frog_jlabels_create(const frog_volume *grid, uint32_t n_images, uint32_t max_labels, uint32_t radius, uint32_t beta, double alpha,
                        int keep_weights, int device, frog_jlabels **out)
{
    size_t total;
    if (int rc = group_arguments("frog_jlabels_create", grid, out, &total)) return rc;
    if (!n_images || n_images > (uint32_t)JL_MAX_N) return fail(FROG_E_INVALID, "frog_jlabels_create: 1 to 32 images");
    if (max_labels > 65536) return fail(FROG_E_INVALID, "frog_jlabels_create: max_labels above 65536");
    if (radius < 1 || radius > 3) return fail(FROG_E_INVALID, "frog_jlabels_create: a radius from 1 to 3");
    if (beta < 1 || beta > 4) return fail(FROG_E_INVALID, "frog_jlabels_create: a beta from 1 to 4");
    if (!(std::isfinite(alpha) && alpha > 0.0)) return fail(FROG_E_INVALID, "frog_jlabels_create: a finite alpha above 0");
    std::unique_ptr<frog_jlabels> a;
    if (int rc = group_new(grid, total, device, a)) return rc;
    a->n_images = n_images;
    a->radius = radius;
    a->beta = beta;
    a->alpha = alpha;
    KCHECK(a->d_target.alloc(total));
    KCHECK(a->d_atlases.alloc((size_t)n_images * total));
    if (keep_weights) KCHECK(a->d_weights.alloc((size_t)n_images * total));
    if (int rc = labels_new_map(a.get(), max_labels ? max_labels : 1024)) return rc;
    KCHECK(a->d_planes.alloc(a->max_labels));
    *out = a.release();
    return FROG_OK;
}

int frog_jlabels_target(frog_jlabels *a, frog_chain *c, const frog_volume *src, int interpolation, double background, frog_volume *resliced)
{
    return wlabels_target("frog_jlabels_target", a, c, src, interpolation, background, resliced);
}

int frog_jlabels_add(frog_jlabels *a, frog_chain *c, const frog_volume *image, const frog_volume *labels, int interpolation,
                     double image_background, double label_background, frog_volume *resliced_image, frog_volume *resliced_labels)
{
    if (!a || !image || !image->data || !frog_volume_voxel_bytes(image->dtype) || !labels || !labels->data)
        return fail(FROG_E_INVALID, "bad arguments to frog_jlabels_add");
    if (!integer_voxel_type(labels->dtype)) return fail(FROG_E_INVALID, "frog_jlabels_add: a label volume has an integer type");
    if (!std::isfinite(image_background) || !std::isfinite(label_background)) return fail(FROG_E_INVALID, "frog_jlabels_add: background is not finite");
    if (!a->has_target) return fail(FROG_E_INVALID, "frog_jlabels_add: before frog_jlabels_target");
    if (a->finished || a->added >= a->n_images) return fail(FROG_E_INVALID, "frog_jlabels_add: more atlases than n_images");
    if (int rc = add_inputs("frog_jlabels_add", a, c, image, resliced_image)) return rc;
    if (int rc = add_inputs("frog_jlabels_add", a, c, labels, resliced_labels)) return rc;
    KCHECK(hipSetDevice(a->device));
    const int rc = with_voxel_type(image->dtype, [&](auto s) {
        return jlabels_add_typed<decltype(s)>(a, c, image, labels, interpolation, image_background, label_background, resliced_image, resliced_labels);
    });
    if (rc == FROG_OK) a->added++;
    return rc;
}

int frog_jlabels_finish(frog_jlabels *a, uint32_t *n_labels)
{
    if (!a || !n_labels) return fail(FROG_E_INVALID, "bad arguments to frog_jlabels_finish");
    if (a->added != a->n_images) return fail(FROG_E_INVALID, "frog_jlabels_finish: fewer atlases added than n_images");
    if (!a->finished) {
        KCHECK(hipSetDevice(a->device));
        if (int rc = jlabels_solve(a)) return rc;
    }
    return frog_wlabels_finish(a, n_labels);        // the table, as for frog_wlabels' scores
}

int frog_jlabels_values(frog_jlabels *a, int64_t *values) { return labels_values("frog_jlabels_values", a, "frog_jlabels_finish", values); }

// frog_jlabels_fused and frog_jlabels_probability answer for their arguments and for finish under their own names; the rest
// is frog_wlabels', under its name
int frog_jlabels_fused(frog_jlabels *a, int64_t fill_label, frog_volume *label, float *confidence)
{
    if (int rc = labels_getter("frog_jlabels_fused", a && (label || confidence) && (!label || label->data), a && a->finished, "frog_jlabels_finish"))
        return rc;
    return frog_wlabels_fused(a, fill_label, label, confidence);
}

int frog_jlabels_probability(frog_jlabels *a, int64_t value, float *p)
{
    if (int rc = labels_getter("frog_jlabels_probability", a && p, a && a->finished, "frog_jlabels_finish")) return rc;
    return frog_wlabels_probability(a, value, p);
}

int frog_jlabels_weight(frog_jlabels *a, uint32_t image_index, float *w)
{
    if (!a || !w) return fail(FROG_E_INVALID, "bad arguments to frog_jlabels_weight");
    if (!a->d_weights.p) return fail(FROG_E_INVALID, "frog_jlabels_weight: the accumulator was created without keep_weights");
    if (!a->finished) return fail(FROG_E_INVALID, "frog_jlabels_weight: before frog_jlabels_finish");
    if (image_index >= a->n_images) return fail(FROG_E_INVALID, "frog_jlabels_weight: no such image");
    KCHECK(hipSetDevice(a->device));
    KCHECK(hipMemcpy(w, a->d_weights.p + (size_t)image_index * a->total, a->total * sizeof(float), hipMemcpyDeviceToHost));
    return FROG_OK;
}

void frog_jlabels_destroy(frog_jlabels *a) { group_destroy(a); }

int frog_distance_map(const frog_volume *labels, int64_t value, int mode, int device, uint32_t *out)
{
    size_t total;
    if (int rc = group_arguments("frog_distance_map", labels, out, &total)) return rc;
    if (!labels->data) return fail(FROG_E_INVALID, "bad arguments to frog_distance_map");
    if (!integer_voxel_type(labels->dtype)) return fail(FROG_E_INVALID, "frog_distance_map: a label volume has an integer type");
    if (mode != 0 && mode != 1) return fail(FROG_E_INVALID, "frog_distance_map: mode 0 (the set) or 1 (its surface)");
    if (!edt_spacing(labels)) return fail(FROG_E_INVALID, "frog_distance_map: the spacing must be positive and finite");
    if (int rc = select_device(device)) return rc;
    return with_integer_voxel_type(labels->dtype, [&](auto s) { return distance_map_typed<decltype(s)>(labels, total, (long long)value, mode, out); });
}

int frog_surface_create(const frog_volume *reference, const int64_t *values, uint32_t n_values, uint32_t percentile, int device,
                        frog_surface **out)
{
    size_t total;
    if (int rc = group_arguments("frog_surface_create", reference, out, &total)) return rc;
    if (!values || !reference->data) return fail(FROG_E_INVALID, "bad arguments to frog_surface_create");
    if (!integer_voxel_type(reference->dtype)) return fail(FROG_E_INVALID, "frog_surface_create: a label volume has an integer type");
    if (!edt_spacing(reference)) return fail(FROG_E_INVALID, "frog_surface_create: the spacing must be positive and finite");
    if (!n_values || n_values > FROG_SURFACE_MAX_LABELS)
        return fail(FROG_E_INVALID, "frog_surface_create: 1 to " + std::to_string(FROG_SURFACE_MAX_LABELS) + " measured values");
    for (uint32_t l = 1; l < n_values; l++)
        if (values[l] <= values[l - 1]) return fail(FROG_E_INVALID, "frog_surface_create: the values must be strictly ascending");
    if (percentile < 1 || percentile > 100) return fail(FROG_E_INVALID, "frog_surface_create: a percentile from 1 to 100");
    std::unique_ptr<frog_surface> a;
    if (int rc = group_new(reference, total, device, a)) return rc;
    a->percentile = percentile;
    a->values.assign(values, values + n_values);
    if (int rc = with_integer_voxel_type(reference->dtype, [&](auto s) { return surface_create_typed<decltype(s)>(a.get(), reference); })) return rc;
    *out = a.release();
    return FROG_OK;
}

int frog_surface_add(frog_surface *a, frog_chain *c, const frog_volume *src, double background, frog_surface_row *rows)
{
    if (!a || !src || !src->data || !rows) return fail(FROG_E_INVALID, "bad arguments to frog_surface_add");
    if (!integer_voxel_type(src->dtype)) return fail(FROG_E_INVALID, "frog_surface_add: a label volume has an integer type");
    if (!std::isfinite(background)) return fail(FROG_E_INVALID, "frog_surface_add: background is not finite");
    if (int rc = add_inputs("frog_surface_add", a, c, src, nullptr)) return rc;
    KCHECK(hipSetDevice(a->device));
    return with_integer_voxel_type(src->dtype, [&](auto s) { return surface_add_typed<decltype(s)>(a, c, src, background, rows); });
}

void frog_surface_destroy(frog_surface *a) { group_destroy(a); }

int frog_modes_planes(const frog_volume *grid, uint32_t n_images, uint32_t n_components, int device, uint32_t *planes)
{
    size_t total;
    if (int rc = modes_arguments("frog_modes_planes", grid, n_images, n_components, planes, &total)) return rc;
    return frog_rank_planes(grid, n_images * n_components, device, planes);        // four bytes per image, component and voxel
}

int frog_modes_create(const frog_volume *grid, uint32_t first_plane, uint32_t n_planes, uint32_t n_images, uint32_t n_components,
                      int device, frog_modes **out)
{
    size_t total;
    if (int rc = modes_arguments("frog_modes_create", grid, n_images, n_components, out, &total)) return rc;
    std::unique_ptr<frog_modes> a;
    if (int rc = windowed_new("frog_modes_create", grid, total, first_plane, n_planes, n_images, device, a)) return rc;
    a->components = n_components;
    KCHECK(a->d_vals.alloc((size_t)n_images * a->window * n_components));
    *out = a.release();
    return FROG_OK;
}

int frog_modes_add_displacement(frog_modes *a, frog_chain *c, const frog_volume *support, const frog_volume *mask)
{
    if (a && a->components != 3) return fail(FROG_E_INVALID, "frog_modes_add_displacement: the accumulator holds one component");
    if (int rc = chain_add_inputs("frog_modes_add_displacement", a, c, support, mask)) return rc;
    KCHECK(hipSetDevice(a->device));
    const uint8_t *d_mask;
    if (int rc = cover_stage_mask("frog_modes_add_displacement", a, mask, &d_mask)) return rc;
    const MaskGrid mg = mask_grid(mask), sg = mask_grid(support);
    const NodeGrid out = node_grid(a->grid.origin, a->grid.spacing, a->grid.dims);
    float *plane = a->d_vals.p + (size_t)a->added * a->window * 3;
    const hipError_t e = chunked_launch(a->window, [&](unsigned blocks, size_t base) {
        modes_displacement_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->first, a->window, c->d_links.p, (int)c->h_links.size(), out, support != nullptr, sg,
                                                            d_mask, mg, plane);
    });
    if (e != hipSuccess) return hip_fail("frog_modes_add_displacement", e);
    return windowed_added("frog_modes_add_displacement", a);
}

int frog_modes_add_jacobian(frog_modes *a, frog_chain *c, const frog_volume *support, const frog_volume *mask, int log_mode)
{
    if (a && a->components != 1) return fail(FROG_E_INVALID, "frog_modes_add_jacobian: the accumulator holds three components");
    if (int rc = chain_add_inputs("frog_modes_add_jacobian", a, c, support, mask)) return rc;
    if (int rc = jacobian_launch("frog_modes_add_jacobian", a, c, support, mask, log_mode, a->first, a->window, a->d_vals.p + (size_t)a->added * a->window))
        return rc;
    return windowed_added("frog_modes_add_jacobian", a);
}

int frog_modes_add(frog_modes *a, frog_chain *c, const frog_volume *src, const frog_volume *mask, int interpolation, double background)
{
    if (a && a->components != 1) return fail(FROG_E_INVALID, "frog_modes_add: the accumulator holds three components");
    return windowed_add<GlmEntry>("frog_modes_add", a, a ? a->d_vals.p : nullptr, c, src, mask, interpolation, background);
}

int frog_modes_plane(frog_modes *a, uint32_t image_index, float *values)
{
    if (!a || !values) return fail(FROG_E_INVALID, "bad arguments to frog_modes_plane");
    if (image_index >= a->added) return fail(FROG_E_INVALID, "frog_modes_plane: that image has not been added");
    KCHECK(hipSetDevice(a->device));
    const size_t stride = a->window * a->components;
    KCHECK(hipMemcpy(values, a->d_vals.p + (size_t)image_index * stride, stride * sizeof(float), hipMemcpyDeviceToHost));
    return FROG_OK;
}

int frog_modes_gram(frog_modes *a, const uint8_t *region, double *gram, uint64_t *n_support)
{
    if (!a || !gram || !n_support) return fail(FROG_E_INVALID, "bad arguments to frog_modes_gram");
    if (int rc = modes_ready("frog_modes_gram", a)) return rc;
    KCHECK(hipSetDevice(a->device));
    const uint32_t n = a->n_images;
    const size_t pairs = (size_t)n * (n + 1) / 2, tiles = (n + MODES_TILE - 1) / MODES_TILE;
    const size_t stride = a->window * a->components;
    const size_t plane_values = (size_t)a->grid.dims[0] * a->grid.dims[1] * a->components, planes = stride / plane_values;
    const size_t chunks = (plane_values + FROG_MODES_CHUNK - 1) / FROG_MODES_CHUNK;
    // a batch of whole planes: its means, its chunk sums and its plane sums
    const size_t plane_bytes = (plane_values + chunks * pairs + pairs) * sizeof(double);
    const size_t batch = std::max<size_t>(1, std::min({ planes, MODES_SCRATCH_BYTES / plane_bytes, MODES_BATCH_CHUNKS / chunks }));
    frog::DevBuf<uint8_t> d_region;
    frog::DevBuf<double> d_mean, d_scratch, d_sums, d_gram;
    frog::DevBuf<unsigned long long> d_count;
    if (int rc = modes_region("frog_modes_gram", a, region, d_region)) return rc;
    KCHECK(d_mean.alloc(batch * plane_values));
    KCHECK(d_scratch.alloc(batch * chunks * pairs));
    KCHECK(d_sums.alloc(batch * pairs));
    KCHECK(d_gram.alloc(pairs));
    KCHECK(d_count.alloc(1));
    KCHECK(hipMemcpy(d_gram.p, gram, pairs * sizeof(double), hipMemcpyHostToDevice));
    KCHECK(hipMemset(d_count.p, 0, sizeof(unsigned long long)));
    hipError_t e = hipSuccess;
    for (size_t first = 0; first < planes && e == hipSuccess; first += batch) {
        const size_t m = std::min(batch, planes - first), v0 = first * plane_values, count = m * plane_values;
        e = chunked_launch(count, [&](unsigned blocks, size_t base) {
            modes_mean_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_vals.p, stride, n, a->components, d_region.p, v0, count, d_mean.p, d_count.p);
        });
        if (e != hipSuccess) break;
        modes_gram_kernel<<<dim3((unsigned)(m * chunks), (unsigned)(tiles * (tiles + 1) / 2)), LAUNCH_BLOCK>>>(
            a->d_vals.p, stride, n, d_mean.p, v0, plane_values, (uint32_t)chunks, d_scratch.p);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        e = chunked_launch(m * pairs, [&](unsigned blocks, size_t base) {
            modes_fold_chunks_kernel<<<blocks, LAUNCH_BLOCK>>>(base, m * pairs, pairs, (uint32_t)chunks, d_scratch.p, d_sums.p);
        });
        if (e != hipSuccess) break;
        e = chunked_launch(pairs, [&](unsigned blocks, size_t base) {
            modes_fold_planes_kernel<<<blocks, LAUNCH_BLOCK>>>(base, pairs, m, d_sums.p, d_gram.p);
        });
    }
    unsigned long long support = 0;
    if (e == hipSuccess) e = hipMemcpy(&support, d_count.p, sizeof support, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gram, d_gram.p, pairs * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("frog_modes_gram", e);
    *n_support += support;
    return FROG_OK;
}

int frog_modes_project(frog_modes *a, const uint8_t *region, uint32_t n_modes, const double *weights, float fill, float *mean, float *modes)
{
    if (!a || !weights || !modes) return fail(FROG_E_INVALID, "bad arguments to frog_modes_project");
    if (int rc = modes_ready("frog_modes_project", a)) return rc;
    if (!n_modes || n_modes > a->n_images) return fail(FROG_E_INVALID, "frog_modes_project: 1 to n_images modes");
    for (size_t e = 0; e < (size_t)n_modes * a->n_images; e++)
        if (!std::isfinite(weights[e])) return fail(FROG_E_INVALID, "frog_modes_project: a weight is not finite");
    KCHECK(hipSetDevice(a->device));
    const uint32_t n = a->n_images;
    const size_t stride = a->window * a->components;
    const size_t batch = std::min(stride, MODES_SCRATCH_BYTES / ((MODES_GROUP + 1) * sizeof(float)) / LAUNCH_BLOCK * LAUNCH_BLOCK);
    frog::DevBuf<uint8_t> d_region;
    frog::DevBuf<double> d_weights;
    frog::DevBuf<float> d_mean, d_modes;
    if (int rc = modes_region("frog_modes_project", a, region, d_region)) return rc;
    KCHECK(d_weights.alloc((size_t)n_modes * n));
    KCHECK(hipMemcpy(d_weights.p, weights, (size_t)n_modes * n * sizeof(double), hipMemcpyHostToDevice));
    KCHECK(d_mean.alloc(batch));
    KCHECK(d_modes.alloc(MODES_GROUP * batch));
    hipError_t e = hipSuccess;
    for (size_t v0 = 0; v0 < stride && e == hipSuccess; v0 += batch) {
        const size_t count = std::min(batch, stride - v0);
        for (uint32_t k0 = 0; k0 < n_modes && e == hipSuccess; k0 += MODES_GROUP) {
            const uint32_t kn = std::min(MODES_GROUP, n_modes - k0);
            float *d_m = mean && !k0 ? d_mean.p : nullptr;
            e = chunked_launch(count, [&](unsigned blocks, size_t base) {
                modes_project_kernel<<<blocks, LAUNCH_BLOCK>>>(base, a->d_vals.p, stride, n, a->components, d_region.p, v0, count, d_weights.p, k0, kn,
                                                               fill, d_m, d_modes.p);
            });
            if (e == hipSuccess && d_m) e = hipMemcpy(mean + v0, d_mean.p, count * sizeof(float), hipMemcpyDeviceToHost);
            for (uint32_t k = 0; k < kn && e == hipSuccess; k++)
                e = hipMemcpy(modes + (size_t)(k0 + k) * stride + v0, d_modes.p + (size_t)k * count, count * sizeof(float), hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess) return hip_fail("frog_modes_project", e);
    return FROG_OK;
}

int frog_modes_eigen(uint32_t n, const double *gram, double divisor, double *values, double *vectors)
{
    if (!gram || !values || !vectors) return fail(FROG_E_INVALID, "bad arguments to frog_modes_eigen");
    if (!n || n > FROG_MODES_MAX_IMAGES) return fail(FROG_E_INVALID, "frog_modes_eigen: 1 to " + std::to_string(FROG_MODES_MAX_IMAGES) + " images");
    if (!(divisor > 0.0) || !std::isfinite(divisor)) return fail(FROG_E_INVALID, "frog_modes_eigen: the divisor must be above 0");
    for (size_t e = 0; e < (size_t)n * (n + 1) / 2; e++)
        if (!std::isfinite(gram[e])) return fail(FROG_E_INVALID, "frog_modes_eigen: a gram entry is not finite");
    std::vector<double> G((size_t)n * n), E((size_t)n * n, 0.0);
    double d = 0.0;
    for (uint32_t i = 0; i < n; i++) {
        E[(size_t)i * n + i] = 1.0;
        for (uint32_t j = 0; j <= i; j++) {
            const double g = gram[(size_t)i * (i + 1) / 2 + j] / divisor;
            G[(size_t)i * n + j] = G[(size_t)j * n + i] = g;
            d = std::max(d, std::fabs(g));
        }
    }
    const double tol = std::ldexp(d, -60);
    // (the off-diagonal norm falls quadratically: a dozen sweeps at most in practice; the bound only rules out an endless loop)
    int sweeps = 0;
    for (bool rotated = true; rotated;) {
        if (++sweeps > 256) return fail(FROG_E_STATE, "frog_modes_eigen: no convergence");
        rotated = false;
        for (uint32_t p = 0; p + 1 < n; p++)
            for (uint32_t q = p + 1; q < n; q++) {
                const double apq = G[(size_t)p * n + q];
                if (!(std::fabs(apq) > tol)) continue;
                rotated = true;
                const double theta = (G[(size_t)q * n + q] - G[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                G[(size_t)p * n + p] -= t * apq;
                G[(size_t)q * n + q] += t * apq;
                G[(size_t)p * n + q] = G[(size_t)q * n + p] = 0.0;
                for (uint32_t k = 0; k < n; k++) {
                    if (k != p && k != q) {
                        const double gkp = G[(size_t)k * n + p], gkq = G[(size_t)k * n + q];
                        G[(size_t)k * n + p] = G[(size_t)p * n + k] = c * gkp - s * gkq;
                        G[(size_t)k * n + q] = G[(size_t)q * n + k] = s * gkp + c * gkq;
                    }
                    const double ekp = E[(size_t)k * n + p], ekq = E[(size_t)k * n + q];
                    E[(size_t)k * n + p] = c * ekp - s * ekq;
                    E[(size_t)k * n + q] = s * ekp + c * ekq;
                }
            }
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return G[(size_t)x * n + x] > G[(size_t)y * n + y]; });
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t col = order[k];
        values[k] = G[(size_t)col * n + col];
        double norm = 0.0, largest = 0.0;
        uint32_t at = 0;
        for (uint32_t i = 0; i < n; i++) {
            const double v = E[(size_t)i * n + col];
            norm += v * v;
            if (std::fabs(v) > largest) { largest = std::fabs(v); at = i; }
        }
        const double scale = (E[(size_t)at * n + col] < 0.0 ? -1.0 : 1.0) / std::sqrt(norm);
        for (uint32_t i = 0; i < n; i++) vectors[(size_t)k * n + i] = E[(size_t)i * n + col] * scale;
    }
    return FROG_OK;
}

void frog_modes_destroy(frog_modes *a) { group_destroy(a); }

}
