// k_tfce.hip.h -- threshold-free cluster enhancement of level maps on one grid (frog_tfce and frog_tfce_volume,
// include/frog_chain.h, which states the results line by line).  Included by chain.hip inside its anonymous namespace, after
// k_ccl.hip.h, whose masks, workspace and kernels it uses as they are.
//
// Levels.  One u8 per voxel and slot, L = trunc(s / dh) saturated at 255, slots `stride` bytes apart: stride is the grid's
// voxels rounded up to a multiple of 32, so a slot starts on a 32-byte boundary and the bytes past the last voxel stay 0.
//
// Enhancement of a batch of slots (one per blockIdx.y, as in k_ccl.hip.h), for k from the batch's highest level down to 1:
// tfce_mask_kernel makes the bit masks L >= k, ccl_label labels them, tfce_accumulate_kernel adds g(extent) * w_k into the f64
// accumulator of every set voxel.  A voxel is set at every k from L(v) down to 1 and at no other, so its accumulator takes
// its terms in descending order of k, one kernel after the other: the sum is the thread's own, no floating-point atomic.
// tfce_round_kernel rounds to f32 and takes the slot's maximum as an integer atomicMax on the bits of a non-negative f32.
#pragma once

// one f32 volume on the device as the levels of one side (glm_level, k_glm.hip.h: the function the fit kernel's level store
// uses), a thread per voxel
__global__ __launch_bounds__(256) void tfce_levels_kernel(size_t base, const float *__restrict__ t, size_t total, uint32_t side, float dh,
                                                          uint8_t *__restrict__ levels)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    levels[v] = glm_level(t[v], side, dh);
}

// the 32 level bytes of mask word w: two 16-byte loads
__device__ __forceinline__ void tfce_load32(const uint8_t *levels, size_t w, uint32_t (&b)[8])
{
    const uint4 *const p = (const uint4 *)(levels + w * 32u);
    const uint4 lo = p[0], hi = p[1];
    b[0] = lo.x; b[1] = lo.y; b[2] = lo.z; b[3] = lo.w;
    b[4] = hi.x; b[5] = hi.y; b[6] = hi.z; b[7] = hi.w;
}

// top[slot] (zero before the launch) = the slot's highest level; a thread per mask word, every lane stays to the end.  The
// maximum only grows, so a wavefront whose own does not exceed the value it loads (at the device's scope) has nothing to add:
// nearly every wavefront of a dense slot would otherwise queue on the slot's one address.
__global__ __launch_bounds__(256) void tfce_top_kernel(size_t base, const uint8_t *__restrict__ levels, size_t stride, size_t words, uint32_t *__restrict__ top)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t m = 0u;
    if (w < words) {
        uint32_t b[8];
        tfce_load32(levels + (size_t)blockIdx.y * stride, w, b);
#pragma unroll
        for (int i = 0; i < 8; i++)
            m = max(max(m, b[i] & 255u), max(max((b[i] >> 8) & 255u, (b[i] >> 16) & 255u), b[i] >> 24));
    }
    for (int step = 32; step >= 1; step >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, step));
    if ((threadIdx.x & 63u) == 0u && m > ccl_load(top + blockIdx.y)) atomicMax(top + blockIdx.y, m);
}

// masks[slot] = the voxels with L >= k, in k_ccl.hip.h's layout; a thread per mask word.  A slot whose highest level is
// below k gets zero words without a load of its levels.
__global__ __launch_bounds__(256) void tfce_mask_kernel(size_t base, const uint8_t *__restrict__ levels, size_t stride, size_t words,
                                                        const uint32_t *__restrict__ top, uint32_t k, uint32_t *__restrict__ masks)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    uint32_t bits = 0u;
    if (top[blockIdx.y] >= k) {
        uint32_t b[8];
        tfce_load32(levels + (size_t)blockIdx.y * stride, w, b);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t four = ((b[i] & 255u) >= k ? 1u : 0u) | (((b[i] >> 8) & 255u) >= k ? 2u : 0u) | (((b[i] >> 16) & 255u) >= k ? 4u : 0u) |
                                  ((b[i] >> 24) >= k ? 8u : 0u);
            bits |= four << (4 * i);
        }
    }
    masks[(size_t)blockIdx.y * words + w] = bits;
}

// After ccl_label on the masks of level k: acc[v] += g(extent of v's component) * weight at every set voxel, g the square root
// (ROOT) or the identity, each product and sum a separately rounded f64 operation.  parent[v] is v's root (ccl_count_kernel
// stored it, in an earlier launch), extent[root] its component's voxels.  A thread per mask word; it leaves on a zero word.
template <bool ROOT>
__global__ __launch_bounds__(256) void tfce_accumulate_kernel(size_t base, const uint32_t *__restrict__ masks, const CclGrid g,
                                                              const uint32_t *__restrict__ parents, const uint32_t *__restrict__ extents,
                                                              double weight, double *__restrict__ accs)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.words) return;
    uint32_t bits = masks[(size_t)blockIdx.y * g.words + w];
    if (!bits) return;
    const uint32_t *const parent = parents + (size_t)blockIdx.y * g.total, *const extent = extents + (size_t)blockIdx.y * g.total;
    double *const acc = accs + (size_t)blockIdx.y * g.total;
    uint32_t last_root = 0xFFFFFFFFu;               // no voxel has this index
    double m = 0.0;
    while (bits) {
        const uint32_t v = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        const uint32_t root = parent[v];
        if (root != last_root) {                    // the neighbours along x mostly share their component
            const double e = (double)extent[root];
            const double ge = ROOT ? sqrt(e) : e;
            m = ge * weight;
            last_root = root;
        }
        acc[v] = acc[v] + m;
    }
}

// tfce = (float)acc, into out (one slot, may be null) and into best[slot] as the largest; a thread per voxel, every lane
// stays to the end.  acc is a sum of non-negative terms, so the f32's bits order as unsigned integers; the atomic is skipped
// as in tfce_top_kernel.
__global__ __launch_bounds__(256) void tfce_round_kernel(size_t base, const double *__restrict__ accs, size_t total, float *__restrict__ out,
                                                         uint32_t *__restrict__ best)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t m = 0u;
    if (v < total) {
        const float f = (float)accs[(size_t)blockIdx.y * total + v];
        if (out) out[v] = f;
        m = __float_as_uint(f);
    }
    for (int step = 32; step >= 1; step >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, step));
    if ((threadIdx.x & 63u) == 0u && m > ccl_load(best + blockIdx.y)) atomicMax(best + blockIdx.y, m);
}
