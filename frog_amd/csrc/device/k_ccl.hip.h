// k_ccl.hip.h -- the connected components of bit masks on one grid (frog_components and frog_clusters, include/frog_chain.h,
// which states the results): union-find on a u32 parent array with integer atomicMin, and extents with integer atomicAdd.
// Included by chain.hip inside its anonymous namespace, after k_glm.hip.h.
//
// Masks.  One bit per voxel, voxel v at bit v & 31 of word v >> 5, `words` = ceil(voxels / 32) words per mask; the bits past
// the last voxel are never set.  The masks of one launch lie `words` apart and are taken one per blockIdx.y, so a thousand
// sparse masks cost a handful of launches.  Every kernel gives a thread one word and leaves at once where the word is zero:
// the parent and extent workspace (one u32 per voxel and mask of the launch, each) is written and read at set voxels only and
// is never cleared.
//
// Components.  ccl_init_kernel makes every set voxel its own parent.  ccl_link_kernel joins a set voxel with each set voxel of
// the forward half of its neighbourhood (the 3, 9 or 13 offsets whose linear index is larger), so every adjacency is seen
// once.  A join walks both voxels to their roots and hangs the larger root below the smaller with atomicMin; a parent is
// never above its child, so when the kernel ends the root of a component is its smallest voxel index, whatever the order the
// joins took.  ccl_count_kernel points every set voxel at its root and adds it to the root's extent: the lanes of a wavefront
// that share a root are counted with a ballot and their leader issues one atomicAdd.  ccl_stats_kernel counts the roots and
// takes the largest extent, reduced over the wavefront before one atomic each.  Every number is an integer sum, minimum or
// maximum: none depends on scheduling.
#pragma once

constexpr uint32_t CCL_BATCH = 64;                  // the most masks one launch labels

struct CclGrid {
    uint32_t nx, ny, nz;
    uint32_t order;                                 // the largest |dx| + |dy| + |dz| of a neighbour: 1, 2 or 3 (6, 18, 26)
    size_t words;                                   // of one mask
    size_t total;                                   // voxels: below 2^32
};

// loads and stores of the parent array while other work-items change it: at the device's scope, past the vector L1
__device__ __forceinline__ uint32_t ccl_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ccl_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t ccl_find(const uint32_t *parent, uint32_t v)
{
    for (;;) {
        const uint32_t p = ccl_load(parent + v);
        if (p == v) return v;
        v = p;
    }
}

// a and b become one tree.  atomicMin on the larger root: where it was a root still, it now hangs below the smaller and the
// join is done; where another join got there first, `old` is the parent it gave, the larger root now hangs below the smaller
// of the two candidates, and the other candidate is joined with b in the next round, so no link is lost.
__device__ __forceinline__ void ccl_join(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = ccl_find(parent, a);
        b = ccl_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t s = a; a = b; b = s; }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void ccl_init_kernel(size_t base, const uint32_t *__restrict__ masks, const CclGrid g, uint32_t *__restrict__ parents,
                                                       uint32_t *__restrict__ extents)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.words) return;
    uint32_t bits = masks[(size_t)blockIdx.y * g.words + w];
    if (!bits) return;
    uint32_t *const parent = parents + (size_t)blockIdx.y * g.total, *const extent = extents + (size_t)blockIdx.y * g.total;
    while (bits) {
        const uint32_t v = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        parent[v] = v;
        extent[v] = 0u;
    }
}

__global__ __launch_bounds__(256) void ccl_link_kernel(size_t base, const uint32_t *__restrict__ masks, const CclGrid g, uint32_t *parents)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.words) return;
    const uint32_t *const mask = masks + (size_t)blockIdx.y * g.words;
    uint32_t bits = mask[w];
    if (!bits) return;
    uint32_t *const parent = parents + (size_t)blockIdx.y * g.total;
    while (bits) {
        const uint32_t v = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        const uint32_t x = v % g.nx, row = v / g.nx, y = row % g.ny, z = row / g.ny;
        for (int dz = 0; dz <= 1; dz++) {
            if (dz && z + 1u >= g.nz) break;
            for (int dy = dz ? -1 : 0; dy <= 1; dy++) {
                if ((dy < 0 && y == 0u) || (dy > 0 && y + 1u >= g.ny)) continue;
                for (int dx = (dz || dy) ? -1 : 1; dx <= 1; dx++) {
                    if ((dx < 0 && x == 0u) || (dx > 0 && x + 1u >= g.nx)) continue;
                    if ((uint32_t)(dz + (dy != 0) + (dx != 0)) > g.order) continue;
                    // the neighbour's index is larger than v's and inside the grid
                    const uint32_t u = (uint32_t)((long long)v + dx + (long long)g.nx * (dy + (long long)g.ny * dz));
                    if ((mask[u >> 5] >> (u & 31u)) & 1u) ccl_join(parent, v, u);
                }
            }
        }
    }
}

// Every lane of the wavefront stays to the end: the ballots count lanes.
__global__ __launch_bounds__(256) void ccl_count_kernel(size_t base, const uint32_t *__restrict__ masks, const CclGrid g, uint32_t *parents,
                                                        uint32_t *extents)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bits = w < g.words ? masks[(size_t)blockIdx.y * g.words + w] : 0u;
    uint32_t *const parent = parents + (size_t)blockIdx.y * g.total, *const extent = extents + (size_t)blockIdx.y * g.total;
    const uint32_t lane = threadIdx.x & 63u;
    constexpr uint32_t NONE = 0xFFFFFFFFu;          // no voxel has this index: grids stay below 2^32 - 1 voxels
    while (__any(bits != 0u)) {
        uint32_t root = NONE;
        if (bits) {
            const uint32_t v = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            root = ccl_find(parent, v);
            ccl_store(parent + v, root);            // a walk that passes here meets the old parent or the root: both lead there
        }
        unsigned long long todo = __ballot(root != NONE);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t theirs = (uint32_t)__shfl((int)root, (int)leader);
            const unsigned long long same = __ballot(root == theirs);
            if (lane == leader) atomicAdd(extent + theirs, (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
}

// stats: per mask the number of components, then the largest extent; zero before the launch
__global__ __launch_bounds__(256) void ccl_stats_kernel(size_t base, const uint32_t *__restrict__ masks, const CclGrid g, const uint32_t *__restrict__ parents,
                                                        const uint32_t *__restrict__ extents, uint32_t *__restrict__ stats)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bits = w < g.words ? masks[(size_t)blockIdx.y * g.words + w] : 0u;
    if (!__any(bits != 0u)) return;
    const uint32_t *const parent = parents + (size_t)blockIdx.y * g.total, *const extent = extents + (size_t)blockIdx.y * g.total;
    uint32_t roots = 0u, largest = 0u;
    while (bits) {
        const uint32_t v = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        if (parent[v] == v) {
            roots++;
            largest = max(largest, extent[v]);
        }
    }
    for (int step = 32; step >= 1; step >>= 1) {
        roots += (uint32_t)__shfl_xor((int)roots, step);
        largest = max(largest, (uint32_t)__shfl_xor((int)largest, step));
    }
    if ((threadIdx.x & 63u) == 0u && roots) {
        atomicAdd(stats + 2u * blockIdx.y, roots);
        atomicMax(stats + 2u * blockIdx.y + 1u, largest);
    }
}

// one mask after ccl_count_kernel, a thread per voxel: root + 1 at a set voxel, 0 elsewhere
__global__ __launch_bounds__(256) void ccl_roots_kernel(size_t base, const uint32_t *__restrict__ mask, size_t total, const uint32_t *__restrict__ parent,
                                                        uint32_t *__restrict__ out)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    out[v] = ((mask[v >> 5] >> (v & 31u)) & 1u) ? parent[v] + 1u : 0u;
}

// one mask as bytes, a thread per voxel
__global__ __launch_bounds__(256) void ccl_bytes_kernel(size_t base, const uint32_t *__restrict__ mask, size_t total, uint8_t *__restrict__ out)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    out[v] = (uint8_t)((mask[v >> 5] >> (v & 31u)) & 1u);
}
