// k_edt.hip.h -- the exact Euclidean distance transform and the surface distances built on it (frog_distance_map,
// frog_surface; include/frog_chain.h states the arithmetic line by line).  Included by chain.hip inside its anonymous
// namespace.
//
// Data.  A label volume on the grid becomes two planes in one pass (edt_surface_kernel): idx[v], 16 bits, the position of
// the voxel's value in the ascending list of measured values (EDT_NONE for any other value), and surf[v], one byte, set
// where one of the six face neighbours carries another value or lies outside the grid.  The features of one transform are
// the voxels with idx == l (mode 0) or with idx == l and surf set (mode 1): no per-label mask is ever written.
//
// The box.  The three passes run inside a box of the grid (EdtBox): the whole grid for frog_distance_map and for the
// reference's maps, the bounding box of A and B for an image's map.  The f64 planes g1 and g2 are indexed by the box, x
// fastest; grid indices are formed from the box's corner.  Every index is a size_t.
//
// x pass.  One wave per line of the box.  The input is binary, so the nearest feature by index is the nearest by
// ((double)(x - q) * sx)^2, and the wave finds it with ballots: a sweep up the line in chunks of 64 voxels carries the last
// feature met and stores the candidate to the left, a sweep down carries the next one and keeps the smaller of the two.  A
// line without a feature ends after the first sweep, +inf throughout; a line with one marks its z-plane (any[k]) and the
// set as a whole (any[nz]).
//
// y and z passes.  One thread per voxel of the box, lanes adjacent in x, so the reads of g[x, q, z] of a wave coalesce for
// every q.  The thread scans q outward from its own index, both directions in one loop, and stops as soon as
// ((double)k * s)^2 alone is >= the best value so far: every later candidate is g + that, g >= 0, so none can be smaller and
// the result is the exact minimum.  A y-line of a plane without a feature, and every line of an empty set, is +inf without
// a scan (any[]).  The z pass ends in the fixed point and either stores it (edt_z_kernel) or, for an image's map, computes
// it only at the reference's surface voxels of the label and collects it there (edt_z_collect_kernel).
//
// Collecting.  n, the sum and the maximum per label are integer atomics, the (key, distance) pairs go to a compact list
// through a counter; a wave first agrees on its takers with a ballot, draws its slots with one atomic and, where all its
// takers carry one label (nearly always), reduces the sum and the maximum with shuffles.  The list's order depends on the
// scheduling; the host takes order statistics of it, which do not.
#pragma once

constexpr uint16_t EDT_NONE = 0xFFFFu;
constexpr int EDT_BOUND_WORDS = 8;              // per label: min x y z, max x y z, surface voxels, unused

static_assert(FROG_SURFACE_MAX_LABELS == 256, "edt_bounds_kernel keeps one LDS slot per label and thread");

struct EdtBox {
    uint32_t x0, y0, z0;            // the box's first voxel in the grid
    uint32_t nx, ny, nz;            // its voxels per axis
    uint32_t gx, gy;                // the grid's voxels along x and y
    double sx, sy, sz;
};

struct EdtList {
    uint2 *entries;                 // (key, distance)
    unsigned long long *count;
};

__device__ __forceinline__ size_t edt_grid_index(const EdtBox &b, uint32_t i, uint32_t j, uint32_t k)
{
    return (size_t)(b.x0 + i) + (size_t)b.gx * ((size_t)(b.y0 + j) + (size_t)b.gy * (size_t)(b.z0 + k));
}

// the stored distance of a squared distance
__device__ __forceinline__ uint32_t edt_fixed(double g)
{
    if (g == std::numeric_limits<double>::infinity()) return 0xFFFFFFFFu;
    const double r = sqrt(g) * 65536.0;
    return r >= 4294967294.0 ? 0xFFFFFFFEu : (uint32_t)llrint(r);
}

// idx and surf of every voxel of a label volume on the grid; `values` ascending, n of them
template <class S>
__global__ __launch_bounds__(256) void edt_surface_kernel(size_t base, const S *__restrict__ labels, uint32_t gx, uint32_t gy, uint32_t gz,
                                                          const long long *__restrict__ values, uint32_t n, uint16_t *__restrict__ idx,
                                                          uint8_t *__restrict__ surf)
{
    const size_t plane = (size_t)gx * gy, total = plane * gz;
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    const uint32_t x = (uint32_t)(v % gx), y = (uint32_t)((v / gx) % gy), z = (uint32_t)(v / plane);
    const S m = labels[v];
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (values[mid] < (long long)m) lo = mid + 1; else hi = mid;
    }
    idx[v] = lo < n && values[lo] == (long long)m ? (uint16_t)lo : EDT_NONE;
    surf[v] = x == 0 || labels[v - 1] != m || x == gx - 1 || labels[v + 1] != m
           || y == 0 || labels[v - gx] != m || y == gy - 1 || labels[v + gx] != m
           || z == 0 || labels[v - plane] != m || z == gz - 1 || labels[v + plane] != m;
}

// Per measured label the bounding box and the number of its surface voxels (the extreme voxels of a set are surface
// voxels, so the box of the surface is the box of the set): LDS atomics per block, then one global atomic per word in use.
// bounds starts as { ~0, ~0, ~0, 0, 0, 0, 0, 0 } per label.
__global__ __launch_bounds__(256) void edt_bounds_kernel(size_t base, const uint16_t *__restrict__ idx, const uint8_t *__restrict__ surf,
                                                         uint32_t gx, uint32_t gy, size_t total, uint32_t *__restrict__ bounds)
{
    __shared__ uint32_t s[EDT_BOUND_WORDS - 1][FROG_SURFACE_MAX_LABELS];
    for (int w = 0; w < EDT_BOUND_WORDS - 1; w++) s[w][threadIdx.x] = w < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < total && surf[v] && idx[v] != EDT_NONE) {
        const uint32_t l = idx[v];
        const uint32_t p[3] = { (uint32_t)(v % gx), (uint32_t)((v / gx) % gy), (uint32_t)(v / ((size_t)gx * gy)) };
        for (int a = 0; a < 3; a++) { atomicMin(&s[a][l], p[a]); atomicMax(&s[3 + a][l], p[a]); }
        atomicAdd(&s[6][l], 1u);
    }
    __syncthreads();
    const uint32_t l = threadIdx.x;
    if (!s[6][l]) return;
    uint32_t *out = bounds + (size_t)l * EDT_BOUND_WORDS;
    for (int a = 0; a < 3; a++) { atomicMin(&out[a], s[a][l]); atomicMax(&out[3 + a], s[3 + a][l]); }
    atomicAdd(&out[6], s[6][l]);
}

// One distance d of label l under `key` into the sums and the list, for the lanes with `take`.  Every lane of the wave
// calls it.
__device__ __forceinline__ void edt_collect(bool take, uint32_t l, uint32_t d, uint32_t key, unsigned long long *__restrict__ sum,
                                            uint32_t *__restrict__ largest, const EdtList list)
{
    const unsigned long long takers = __ballot(take);
    if (!takers) return;                                // wave-uniform
    const uint32_t lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)takers) - 1;
    unsigned long long slot = 0;
    if ((int)lane == leader) slot = atomicAdd(list.count, (unsigned long long)__popcll(takers));
    slot = __shfl(slot, leader);
    if (take) list.entries[slot + __popcll(takers & ((1ull << lane) - 1))] = make_uint2(key, d);
    const uint32_t l0 = __shfl(l, leader);
    if (!__ballot(take && l != l0)) {
        unsigned long long s = take ? d : 0u;
        uint32_t m = take ? d : 0u;
        for (int h = 32; h > 0; h >>= 1) {
            s += __shfl_xor(s, h);
            const uint32_t o = __shfl_xor(m, h);
            m = o > m ? o : m;
        }
        if ((int)lane == leader) { atomicAdd(&sum[l0], s); atomicMax(&largest[l0], m); }
    } else if (take) {
        atomicAdd(&sum[l], (unsigned long long)d);
        atomicMax(&largest[l], d);
    }
}

// The image's side of an add: D_B[label(v)][v] at every surface voxel v of the image that carries a measured label.
__global__ __launch_bounds__(256) void edt_read_kernel(size_t base, const uint16_t *__restrict__ idx, const uint8_t *__restrict__ surf,
                                                       size_t total, const uint32_t *__restrict__ maps, unsigned long long *__restrict__ sum,
                                                       uint32_t *__restrict__ largest, const EdtList list)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool take = v < total && surf[v] && idx[v] != EDT_NONE;
    const uint32_t l = take ? idx[v] : 0u;
    const uint32_t d = take ? maps[(size_t)l * total + v] : 0u;
    edt_collect(take, l, d, l, sum, largest, list);
}

__device__ __forceinline__ bool edt_feature(const uint16_t *__restrict__ idx, const uint8_t *__restrict__ surf, size_t v, uint32_t l,
                                            int surface_only)
{
    return idx[v] == l && (!surface_only || surf[v]);
}

__device__ __forceinline__ double edt_square(long long k, double s)
{
    const double d = (double)k * s;
    return d * d;
}

// g1 of the box; one wave per line, 64 work-items per line.  any[] is zero before the launch.
__global__ __launch_bounds__(256) void edt_x_kernel(size_t base, const EdtBox b, const uint16_t *__restrict__ idx,
                                                    const uint8_t *__restrict__ surf, uint32_t l, int surface_only,
                                                    double *__restrict__ g1, uint32_t *__restrict__ any)
{
    const size_t line = (base + (size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (line >= (size_t)b.ny * b.nz) return;            // wave-uniform: base is a multiple of 256
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t j = (uint32_t)(line % b.ny), k = (uint32_t)(line / b.ny);
    const size_t from = edt_grid_index(b, 0, j, k), to = line * b.nx;
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;    // lanes 0 .. lane
    long long last = -1;
    for (uint32_t c = 0; c < b.nx; c += 64) {
        const uint32_t i = c + lane;
        const bool f = i < b.nx && edt_feature(idx, surf, from + i, l, surface_only);
        const unsigned long long mask = __ballot(f), below = mask & upto;
        const long long q = below ? (long long)c + 63 - __clzll((long long)below) : last;
        if (i < b.nx) g1[to + i] = q >= 0 ? edt_square((long long)i - q, b.sx) : std::numeric_limits<double>::infinity();
        if (mask) last = (long long)c + 63 - __clzll((long long)mask);
    }
    if (last < 0) return;
    if (lane == 0) { any[k] = 1u; any[b.nz] = 1u; }
    long long next = -1;
    for (uint32_t c = (b.nx - 1) / 64 * 64;; c -= 64) {
        const uint32_t i = c + lane;
        const bool f = i < b.nx && edt_feature(idx, surf, from + i, l, surface_only);
        const unsigned long long mask = __ballot(f), above = mask & (~0ull << lane);
        const long long q = above ? (long long)c + __ffsll((long long)above) - 1 : next;
        if (i < b.nx && q >= 0) {
            const double r = edt_square((long long)i - q, b.sx);
            if (r < g1[to + i]) g1[to + i] = r;
        }
        if (mask) next = (long long)c + __ffsll((long long)mask) - 1;
        if (c == 0) break;
    }
}

// min over q in [0, n) of ( g[q * stride] + ((double)(at - q) * s)^2 ), g read from `line`
__device__ __forceinline__ double edt_scan(const double *__restrict__ line, size_t stride, uint32_t at, uint32_t n, double s)
{
    double best = line[(size_t)at * stride] + 0.0;
    for (uint32_t k = 1; k <= at || k < n - at; k++) {
        const double w = edt_square((long long)k, s);
        if (w >= best) break;
        if (k <= at) {
            const double c = line[(size_t)(at - k) * stride] + w;
            if (c < best) best = c;
        }
        if (k < n - at) {
            const double c = line[(size_t)(at + k) * stride] + w;
            if (c < best) best = c;
        }
    }
    return best;
}

__global__ __launch_bounds__(256) void edt_y_kernel(size_t base, const EdtBox b, const double *__restrict__ g1, double *__restrict__ g2,
                                                    const uint32_t *__restrict__ any)
{
    const size_t plane = (size_t)b.nx * b.ny, total = plane * b.nz;
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    const uint32_t i = (uint32_t)(v % b.nx), j = (uint32_t)((v / b.nx) % b.ny), k = (uint32_t)(v / plane);
    g2[v] = any[k] ? edt_scan(g1 + (size_t)k * plane + i, b.nx, j, b.ny, b.sy) : std::numeric_limits<double>::infinity();
}

// g3 as the stored distance, at every voxel of the box; `out` is indexed by the box
__global__ __launch_bounds__(256) void edt_z_kernel(size_t base, const EdtBox b, const double *__restrict__ g2, const uint32_t *__restrict__ any,
                                                    uint32_t *__restrict__ out)
{
    const size_t plane = (size_t)b.nx * b.ny, total = plane * b.nz;
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    const uint32_t k = (uint32_t)(v / plane);
    out[v] = any[b.nz] ? edt_fixed(edt_scan(g2 + v % plane, plane, k, b.nz, b.sz)) : 0xFFFFFFFFu;
}

// The reference's side of an add for label l: g3 of the image's surface only where the reference has a surface voxel of the
// label, collected under `key`.  The caller launches it only for a label whose image surface is not empty.
__global__ __launch_bounds__(256) void edt_z_collect_kernel(size_t base, const EdtBox b, const double *__restrict__ g2,
                                                            const uint16_t *__restrict__ ref_idx, const uint8_t *__restrict__ ref_surf,
                                                            uint32_t l, uint32_t key, unsigned long long *__restrict__ sum,
                                                            uint32_t *__restrict__ largest, const EdtList list)
{
    const size_t plane = (size_t)b.nx * b.ny, total = plane * b.nz;
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool take = false;
    uint32_t d = 0;
    if (v < total) {
        const uint32_t i = (uint32_t)(v % b.nx), j = (uint32_t)((v / b.nx) % b.ny), k = (uint32_t)(v / plane);
        const size_t at = edt_grid_index(b, i, j, k);
        take = ref_surf[at] && ref_idx[at] == l;
        if (take) d = edt_fixed(edt_scan(g2 + v % plane, plane, k, b.nz, b.sz));
    }
    edt_collect(take, l, d, key, sum, largest, list);
}
