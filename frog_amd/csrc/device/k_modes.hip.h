// k_modes.hip.h -- the principal modes of a registered group (frog_modes, include/frog_chain.h, which states the arithmetic line
// by line): the displacement add, the mean of a batch of values, the Gram kernel with its two folds, and the projection.
// Included by chain.hip inside its anonymous namespace, after k_glm.hip.h, whose scalar adds frog_modes reuses as they are.
//
// Store.  Image i owns `stride` = window voxels x components consecutive floats, a voxel's components next to each other: a
// VALUE is one float of that plane, and everything below works on values, v in [0, stride).  A voxel's components take part
// together, so "every image takes part" is tested per value.
//
// Gram.  An f64 rank-k update in a stated order.  The order was chosen so that no sum crosses lanes: a thread owns
// the sums of its pairs over one CHUNK of FROG_MODES_CHUNK values, and it is whole chunk sums that are added afterwards.
//   modes_mean_kernel   one thread per value of the batch: m, or a NaN outside the support; counts the support voxels with
//                       one integer atomic per block.
//   modes_gram_kernel   block (chunk, tile pair (I, J), J <= I), tiles of MODES_TILE images.  The block stages c_i = x_i - m of
//                       both tiles for MODES_STEP values in LDS (+0.0 outside the support, beyond the chunk's end and for images
//                       beyond n: such a term adds +0.0, and no sum here is ever -0.0, so it changes no bit), then every thread
//                       that owns a 2 x 2 block of pairs adds its MODES_STEP products in value order: two ds_read_b128 per 8
//                       flops.  Only the blocks with an entry of the lower triangle are dealt out, to the first threads.  Rows
//                       are padded to MODES_ROW doubles: the staging writes of consecutive values fall into different banks
//                       and a row stays 16-byte aligned.  The chunk's sums go to scratch[chunk][pair].
//   modes_fold_chunks_kernel  one thread per (plane of the batch, pair): the plane's chunk sums ascending, from +0.0.
//   modes_fold_planes_kernel  one thread per pair: the batch's plane sums ascending onto gram.
// Plain vector f64 multiplies and adds; the matrix cores are left out because the order in which v_mfma_f64 adds its four
// products is not documented.  No floating-point atomic.
//
// Projection.  One thread per value: m as above, then one pass over the images per group of MODES_GROUP modes, the group's
// sums in registers, the weights read with wave-uniform addresses.
#pragma once

constexpr uint32_t MODES_TILE = 32;                 // images of a tile
constexpr uint32_t MODES_STEP = 32;                 // values staged at a time
constexpr uint32_t MODES_ROW = MODES_TILE + 2;      // doubles of a staged value's row
constexpr uint32_t MODES_GROUP = 8;                 // modes of one projection launch
static_assert(FROG_MODES_CHUNK % MODES_STEP == 0, "a chunk is whole steps");
static_assert(MODES_TILE * MODES_TILE == 4 * 256, "256 threads own 2 x 2 pairs each");

// The displacement chain_sample_kernel stores for the node (grid_node, chain_point<false>, position minus node), cast once to
// f32, with glm_jacobian_kernel's validity.
__global__ __launch_bounds__(256) void modes_displacement_kernel(size_t base, size_t first, size_t window, const DevLink *links, int n_links,
                                                                 const NodeGrid out, int has_support, const MaskGrid support,
                                                                 const uint8_t *__restrict__ mask, const MaskGrid mg, float *__restrict__ plane)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= window) return;
    const size_t idx = first + w;
    double p[3], c[3], A[3][3];
    grid_node(out, idx, p);
    const double node[3] = { p[0], p[1], p[2] };
    chain_point<false>(links, n_links, p, A);
    bool valid = !has_support || voxel_coordinates(p, support.so, support.ss, support.sx, support.sy, support.sz, c);
    if (valid && mask) valid = mask_covers(p, mask, mg);
    const float x[3] = { (float)(p[0] - node[0]), (float)(p[1] - node[1]), (float)(p[2] - node[2]) };
    valid = valid && x[0] - x[0] == 0.0f && x[1] - x[1] == 0.0f && x[2] - x[2] == 0.0f;
    for (int k = 0; k < 3; k++) plane[3 * w + k] = valid ? x[k] : __uint_as_float(GLM_NAN_BITS);
}

// m of value v, and whether v lies in the support
__device__ __forceinline__ bool modes_mean(const float *__restrict__ vals, size_t stride, uint32_t n, uint32_t components,
                                           const uint8_t *__restrict__ region, size_t v, double *m)
{
    bool in = !region || region[v / components] != 0;
    double s = 0.0;
#pragma unroll 4
    for (uint32_t i = 0; i < n; i++) {
        const float x = vals[(size_t)i * stride + v];
        in = in && __float_as_uint(x) != GLM_NAN_BITS;
        s = s + (double)x;
    }
    *m = s / (double)n;
    return in;
}

// mean[t] of the `count` values from v0 on: m, or a NaN outside the support
__global__ __launch_bounds__(256) void modes_mean_kernel(size_t base, const float *__restrict__ vals, size_t stride, uint32_t n, uint32_t components,
                                                         const uint8_t *__restrict__ region, size_t v0, size_t count,
                                                         double *__restrict__ mean, unsigned long long *__restrict__ n_support)
{
    const size_t t = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool counts = false;
    if (t < count) {
        double m;
        const bool in = modes_mean(vals, stride, n, components, region, v0 + t, &m);
        mean[t] = in ? m : __longlong_as_double(0x7FF8000000000000ll);
        counts = in && (v0 + t) % components == 0;
    }
    const int voxels = __syncthreads_count(counts);
    if (threadIdx.x == 0 && voxels) atomicAdd(n_support, (unsigned long long)voxels);
}

// c of MODES_STEP values of one tile into `rows`: thread t stages value t % MODES_STEP of images t / MODES_STEP + 8 r
__device__ __forceinline__ void modes_stage(double *rows, const float *__restrict__ vals, size_t stride, uint32_t n, uint32_t tile,
                                            const double *__restrict__ mean, size_t v0, size_t at, size_t end)
{
    const uint32_t value = threadIdx.x % MODES_STEP;
    const size_t t = at + value;
    const double m = t < end ? mean[t] : __longlong_as_double(0x7FF8000000000000ll);
    for (uint32_t r = 0; r < MODES_TILE * MODES_STEP / 256; r++) {
        const uint32_t local = threadIdx.x / MODES_STEP + r * (256 / MODES_STEP), image = tile * MODES_TILE + local;
        double c = 0.0;
        if (m == m && image < n) c = (double)vals[(size_t)image * stride + v0 + t] - m;
        rows[value * MODES_ROW + local] = c;
    }
}

// scratch[chunk][pair]: the chunk sums of the batch's chunks.  The batch is `planes` whole z-planes of plane_values values each,
// from value v0 of the window on; `mean` is the batch's.  blockIdx.x: the chunk, blockIdx.y: the tile pair.
__global__ __launch_bounds__(256) void modes_gram_kernel(const float *__restrict__ vals, size_t stride, uint32_t n, const double *__restrict__ mean,
                                                         size_t v0, size_t plane_values, uint32_t chunks_per_plane, double *__restrict__ scratch)
{
    __shared__ __attribute__((aligned(16))) double rows_i[MODES_STEP * MODES_ROW];
    __shared__ __attribute__((aligned(16))) double rows_j[MODES_STEP * MODES_ROW];
    uint32_t I = 0;
    while ((I + 1) * (I + 2) / 2 <= blockIdx.y) I++;
    const uint32_t J = blockIdx.y - I * (I + 1) / 2;
    const size_t plane = blockIdx.x / chunks_per_plane, chunk = blockIdx.x % chunks_per_plane;
    const size_t begin = plane * plane_values + chunk * FROG_MODES_CHUNK;
    const size_t end = plane * plane_values + min((chunk + 1) * (size_t)FROG_MODES_CHUNK, plane_values);
    // The 2 x 2 blocks of pairs that hold an entry of the lower triangle, dealt to the first threads: with few images, and on a
    // diagonal tile pair, whole wavefronts own nothing and only stage.
    const uint32_t blocks_i = (min(MODES_TILE, n - I * MODES_TILE) + 1) / 2, blocks_j = (min(MODES_TILE, n - J * MODES_TILE) + 1) / 2;
    const bool works = threadIdx.x < (I == J ? blocks_i * (blocks_i + 1) / 2 : blocks_i * blocks_j);
    uint32_t ti = 0, tj = 0;
    if (works && I == J) {
        while ((ti + 1) * (ti + 2) / 2 <= threadIdx.x) ti++;
        tj = threadIdx.x - ti * (ti + 1) / 2;
    } else if (works) {
        ti = threadIdx.x / blocks_j;
        tj = threadIdx.x % blocks_j;
    }
    const double *own_j = I == J ? rows_i : rows_j;
    double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
    for (size_t at = begin; at < end; at += MODES_STEP) {
        modes_stage(rows_i, vals, stride, n, I, mean, v0, at, end);
        if (I != J) modes_stage(rows_j, vals, stride, n, J, mean, v0, at, end);
        __syncthreads();
#pragma unroll 8
        for (uint32_t value = 0; works && value < MODES_STEP; value++) {
            const double2 a = *(const double2 *)&rows_i[value * MODES_ROW + 2 * ti];
            const double2 b = *(const double2 *)&own_j[value * MODES_ROW + 2 * tj];
            double p;
            p = a.x * b.x; s00 = s00 + p;
            p = a.x * b.y; s01 = s01 + p;
            p = a.y * b.x; s10 = s10 + p;
            p = a.y * b.y; s11 = s11 + p;
        }
        __syncthreads();
    }
    const size_t pairs = (size_t)n * (n + 1) / 2;
    double *out = scratch + (size_t)blockIdx.x * pairs;
    const uint32_t i = I * MODES_TILE + 2 * ti, j = J * MODES_TILE + 2 * tj;
    if (!works) return;
    if (i < n && j <= i) out[(size_t)i * (i + 1) / 2 + j] = s00;
    if (i < n && j + 1 <= i) out[(size_t)i * (i + 1) / 2 + j + 1] = s01;
    if (i + 1 < n && j <= i + 1) out[(size_t)(i + 1) * (i + 2) / 2 + j] = s10;
    if (i + 1 < n && j + 1 <= i + 1) out[(size_t)(i + 1) * (i + 2) / 2 + j + 1] = s11;
}

// plane_sums[plane][pair] = the plane's chunk sums ascending, from +0.0; e indexes (plane, pair), pair fastest
__global__ __launch_bounds__(256) void modes_fold_chunks_kernel(size_t base, size_t total, size_t pairs, uint32_t chunks_per_plane,
                                                                const double *__restrict__ scratch, double *__restrict__ plane_sums)
{
    const size_t e = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t plane = e / pairs, pair = e % pairs;
    const double *from = scratch + plane * chunks_per_plane * pairs + pair;
    double t = 0.0;
    for (uint32_t k = 0; k < chunks_per_plane; k++) t = t + from[(size_t)k * pairs];
    plane_sums[e] = t;
}

// gram[pair] = gram[pair] + the batch's plane sums, ascending
__global__ __launch_bounds__(256) void modes_fold_planes_kernel(size_t base, size_t pairs, size_t planes, const double *__restrict__ plane_sums,
                                                                double *__restrict__ gram)
{
    const size_t pair = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= pairs) return;
    double g = gram[pair];
    for (size_t k = 0; k < planes; k++) g = g + plane_sums[k * pairs + pair];
    gram[pair] = g;
}

// The `count` values from v0 on: mean (null: not wanted) and the modes k0 .. k0 + kn - 1 (kn <= MODES_GROUP) into
// modes[k * count + t]; weights is n_modes x n on the device.
__global__ __launch_bounds__(256) void modes_project_kernel(size_t base, const float *__restrict__ vals, size_t stride, uint32_t n, uint32_t components,
                                                            const uint8_t *__restrict__ region, size_t v0, size_t count,
                                                            const double *__restrict__ weights, uint32_t k0, uint32_t kn, float fill,
                                                            float *__restrict__ mean, float *__restrict__ modes)
{
    const size_t t = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    double m;
    const bool in = modes_mean(vals, stride, n, components, region, v0 + t, &m);
    double s[MODES_GROUP];
    for (uint32_t k = 0; k < MODES_GROUP; k++) s[k] = 0.0;
    if (in) {
        const double *w = weights + (size_t)k0 * n;
#pragma unroll 2
        for (uint32_t i = 0; i < n; i++) {
            const double c = (double)vals[(size_t)i * stride + v0 + t] - m;
#pragma unroll
            for (uint32_t k = 0; k < MODES_GROUP; k++) {
                if (k < kn) {
                    const double p = w[(size_t)k * n + i] * c;
                    s[k] = s[k] + p;
                }
            }
        }
    }
    if (mean) mean[t] = in ? (float)m : fill;
#pragma unroll
    for (uint32_t k = 0; k < MODES_GROUP; k++)
        if (k < kn) modes[(size_t)k * count + t] = in ? (float)s[k] : fill;
}
