// k_smooth.hip.h -- the coverage-aware Gaussian of frog_smooth_volume and frog_glm_smooth (include/frog_chain.h, which states
// the arithmetic line by line): a normalised convolution over the voxels that take part, as three separable passes over two
// f64 fields, num and den.
// Included by chain.hip inside its anonymous namespace, after k_glm.hip.h, whose NaN marks a voxel that does not take part.
//
// Mapping.  A RANGE is whole z-planes of the grid: the planes a window needs, the window extended by R_z planes on each side
// and clipped at the grid's ends.  One thread per voxel in every pass, consecutive threads at consecutive x, so every load
// and store of a wavefront is one contiguous run whichever axis the pass walks:
//   smooth_x_kernel  reads the f32 values (and the flags) of the range along x and forms num and den on the fly: the two
//                    fields never exist unconvolved.  Writes one double2 (num, den) per voxel of the range.
//   smooth_y_kernel  reads double2 at e + d * nx, writes double2.
//   smooth_z_kernel  runs over the WINDOW alone, reads double2 at e + d * nx * ny inside the range, divides and writes the
//                    final f32: the z pass's f64 result is never stored.
// So the scratch is 4 + 16 + 16 bytes per voxel of the range, and HBM sees each field once per pass: a voxel's 2 R + 1 taps
// are its neighbours' loads, which the caches serve.
// A pass's loop runs d = -R .. +R in every lane alike, so the tap w_|d| has a wave-uniform address and is read from the
// kernel's arguments by a scalar load.  A neighbour outside the grid, or one that does not take part, enters as (+0.0, +0.0)
// through a select, never through a branch around the addition: no sum here is ever -0.0 (each starts from +0.0 and
// x + (-x) is +0.0), so adding +0.0 changes no bit and the sums carry the bits of the loop over the grid's own neighbours.
// The loops are unrolled four times so that four loads are in flight per thread; the additions keep their order.
// Every line is one rounded f64 operation (-ffp-contract=off).  No atomics: a voxel's sums are its own.
#pragma once

struct SmoothTaps {
    uint32_t radius;
    double w[FROG_SMOOTH_MAX_RADIUS + 1];
};

// does voxel e of the range take part: its flag (where there are flags) and a finite value
__device__ __forceinline__ bool smooth_takes(const float *__restrict__ raw, const uint8_t *__restrict__ take, size_t e)
{
    const float v = raw[e];
    return (!take || take[e] != 0) && v - v == 0.0f;
}

__global__ __launch_bounds__(256) void smooth_x_kernel(size_t base, size_t count, uint32_t nx, const float *__restrict__ raw,
                                                       const uint8_t *__restrict__ take, const SmoothTaps t, double2 *__restrict__ out)
{
    const size_t e = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const int x = (int)((uint32_t)e % nx), R = (int)t.radius;      // a range holds at most 2^31 voxels
    double num = 0.0, den = 0.0;
#pragma unroll 4
    for (int d = -R; d <= R; d++) {
        const double w = t.w[d < 0 ? -d : d];
        const bool inside = x + d >= 0 && x + d < (int)nx;
        const size_t at = inside ? (size_t)((long long)e + d) : e;
        const bool on = inside && smooth_takes(raw, take, at);
        const double a = on ? (double)raw[at] : 0.0, b = on ? 1.0 : 0.0;
        double m = w * a;
        num = num + m;
        m = w * b;
        den = den + m;
    }
    out[e] = make_double2(num, den);
}

__global__ __launch_bounds__(256) void smooth_y_kernel(size_t base, size_t count, uint32_t nx, uint32_t ny, const double2 *__restrict__ in,
                                                       const SmoothTaps t, double2 *__restrict__ out)
{
    const size_t e = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const int y = (int)((uint32_t)e / nx % ny), R = (int)t.radius;
    double num = 0.0, den = 0.0;
#pragma unroll 4
    for (int d = -R; d <= R; d++) {
        const double w = t.w[d < 0 ? -d : d];
        const bool inside = y + d >= 0 && y + d < (int)ny;
        const double2 v = in[inside ? (size_t)((long long)e + (long long)d * nx) : e];
        const double a = inside ? v.x : 0.0, b = inside ? v.y : 0.0;
        double m = w * a;
        num = num + m;
        m = w * b;
        den = den + m;
    }
    out[e] = make_double2(num, den);
}

// `offset` is the window's first voxel in the range, `count` the range's voxels: a plane outside the range lies outside the grid
__global__ __launch_bounds__(256) void smooth_z_kernel(size_t base, size_t window, size_t offset, size_t count, size_t plane,
                                                       const float *__restrict__ raw, const uint8_t *__restrict__ take,
                                                       const double2 *__restrict__ in, const SmoothTaps t, float *__restrict__ out)
{
    const size_t i = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= window) return;
    const size_t e = offset + i;
    const int R = (int)t.radius;
    double num = 0.0, den = 0.0;
#pragma unroll 4
    for (int d = -R; d <= R; d++) {
        const double w = t.w[d < 0 ? -d : d];
        const long long to = (long long)e + (long long)d * (long long)plane;
        const bool inside = to >= 0 && to < (long long)count;
        const double2 v = in[inside ? (size_t)to : e];
        const double a = inside ? v.x : 0.0, b = inside ? v.y : 0.0;
        double m = w * a;
        num = num + m;
        m = w * b;
        den = den + m;
    }
    const double q = num / den;
    out[i] = smooth_takes(raw, take, e) ? (float)q : __uint_as_float(GLM_NAN_BITS);
}
