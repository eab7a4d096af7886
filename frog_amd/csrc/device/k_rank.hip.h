// k_rank.hip.h -- per-voxel order statistics over the images of a group (frog_rank, include/frog_chain.h): the collect
// kernels, which store one sort key per voxel and add, and the two finish kernels, which sort a voxel's keys and select.
// Included by chain.hip inside its anonymous namespace, after the reslice and cover device code it reuses.
//
// Keys.  key(x) of x = (float)r: ~u where the sign bit of u = bits(x) is set, else u ^ 0x80000000; unsigned order of the keys
// is -inf < ... < -0 < +0 < ... < +inf < NaNs of positive sign, and 0xFFFFFFFF is the key of a NaN, so a participating value
// never has it: it marks "does not take part" and sorts last.  Nothing here is rounded except where the header states one
// f64 or f32 operation, so every method that sorts gives the same bits: the two tiers below agree by construction.
//
// Finish, tier 1 (n_images <= RANK_REG_MAX): one thread per voxel, the keys in P = 8 .. 64 registers, a fully unrolled
// bitonic network of compare-exchanges (v_min_u32 / v_max_u32), every index a compile-time constant.  a[lo] and a[hi]
// depend on k, so they are picked with an unrolled compare-and-select over the P registers.
// Finish, tier 2 (up to FROG_RANK_MAX_IMAGES): one block of 256 threads per tile of T = 16384 / P consecutive voxels,
// 64 KiB of LDS, so two blocks fit a CU.  Key n of voxel t sits at word n * T + t: the global loads are runs of T keys per
// image plane, and the threads of a wavefront that work on the same network position of neighbouring voxels touch
// consecutive words.  The same network, one compare-exchange per thread and step, a barrier between steps; thread t < T then
// selects for voxel t.
#pragma once

constexpr uint32_t RANK_SENTINEL = 0xFFFFFFFFu;
constexpr uint32_t RANK_REG_MAX = 64;               // the largest n_images of the register tier (P = 128 spills scalar registers)
constexpr uint32_t RANK_LDS_KEYS = 16384;           // keys per block of the LDS tier: 64 KiB
constexpr uint32_t RANK_MAX_Q = 16;

static_assert(FROG_RANK_MAX_IMAGES == 4096, "the LDS tier's largest padded size is 4096 keys");

__device__ __forceinline__ uint32_t rank_key(float x)
{
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

__device__ __forceinline__ float rank_key_value(uint32_t key)
{
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// what an add stores for a voxel: the key of x where the voxel is valid and x is not NaN
__device__ __forceinline__ uint32_t rank_entry(bool valid, float x)
{
    return valid && x == x ? rank_key(x) : RANK_SENTINEL;
}

// The collect kernels of the accumulators that keep a plane per image over a window (frog_rank and frog_glm, k_glm.hip.h)
// store Entry::of(valid, x) as an Entry::type: this one the key.
struct RankEntry {
    using type = uint32_t;
    static __device__ __forceinline__ type of(bool valid, float x) { return rank_entry(valid, x); }
};

// cover_reslice_kernel with the store of Entry in place of cover_update: window voxel w is voxel `first + w` of the whole
// grid, and its position is computed from that index, so a window gives what the whole grid gives there
template <class S, class Entry>
__global__ __launch_bounds__(256) void window_reslice_kernel(size_t base, size_t first, size_t window, const DevLink *links, int n_links,
                                                             const S *__restrict__ src, const ResliceGrid g, const uint8_t *__restrict__ mask,
                                                             const MaskGrid mg, typename Entry::type *__restrict__ plane)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= window) return;
    const size_t idx = first + w;
    double p[3], c[3];
    reslice_position(links, n_links, g.out, idx, p);
    bool valid = voxel_coordinates(p, g.so, g.ss, g.sx, g.sy, g.sz, c);
    const S r = reslice_sample<S>(src, g, c, valid);
    if (valid && mask) valid = mask_covers(p, mask, mg);
    plane[w] = Entry::of(valid, (float)r);
}

// a source (and a mask) already on the grid: every voxel is inside
template <class S, class Entry>
__global__ __launch_bounds__(256) void window_identity_kernel(size_t base, size_t first, size_t window, const S *__restrict__ src,
                                                              const uint8_t *__restrict__ mask, typename Entry::type *__restrict__ plane)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= window) return;
    const size_t idx = first + w;
    plane[w] = Entry::of(!mask || mask[idx] != 0, (float)src[idx]);
}

// the arguments of a finish that both tiers take by value
struct RankFinish {
    size_t window;              // voxels of the window = the stride between image planes
    uint32_t n;                 // planes filled
    uint32_t min_count;
    float fill;
    uint32_t n_q;               // probabilities asked for: q[0 .. n_q)
    int sort;                   // 0: only the count is wanted
    double q[RANK_MAX_Q];
    float *quantiles;           // n_q planes, or null when n_q == 0
    float *mad;                 // may be null
    uint16_t *count;            // may be null
};

// The value at probability q of k >= 1 ascending values, as the header states it.  get(lo, hi, &a, &b) fetches the keys at
// those two positions; DIST: the keys are the bits of non-negative floats (the second sort), else rank_key's.  A NaN result
// (inf - inf between neighbours of opposite sign) is stored as the quiet NaN 0x7FC00000.
template <bool DIST, class Get>
__device__ __forceinline__ float rank_quantile(double q, uint32_t k, Get get)
{
    const double h = q * (double)(k - 1u);
    const double fl = floor(h);
    const double f = h - fl;
    const uint32_t lo = (uint32_t)fl;
    const uint32_t hi = lo + 1u < k ? lo + 1u : k - 1u;
    uint32_t key_lo, key_hi;
    get(lo, hi, key_lo, key_hi);
    const float a = DIST ? __uint_as_float(key_lo) : rank_key_value(key_lo);
    const float b = DIST ? __uint_as_float(key_hi) : rank_key_value(key_hi);
    if (f == 0.0 || a == b) return a;
    const double da = (double)a, db = (double)b;
    const double diff = db - da;
    const double part = f * diff;
    const double sum = da + part;
    const float r = (float)sum;
    return r == r ? r : __uint_as_float(0x7FC00000u);
}

// the key a value takes in the second sort: the bits of |x - m|, one f32 subtraction
__device__ __forceinline__ uint32_t rank_distance(uint32_t key, float m)
{
    const float d = rank_key_value(key) - m;
    return __float_as_uint(fabsf(d));
}

// ---- tier 1: the keys of a voxel in registers -----------------------------------------------------------------------------

// One step of the network over P registers.  FIRST: the opening step of a merge of runs of K2 / 2, position i against
// i ^ (K2 - 1); otherwise i against i ^ J.  Every exchange is ascending.
template <int P, int K2, int J, bool FIRST>
__device__ __forceinline__ void rank_net_step(uint32_t (&key)[P])
{
#pragma unroll
    for (int i = 0; i < P; i++) {
        const int l = FIRST ? (i ^ (K2 - 1)) : (i ^ J);
        if (l > i) {
            const uint32_t a = key[i], b = key[l];
            key[i] = min(a, b);
            key[l] = max(a, b);
        }
    }
}

template <int P, int K2, int J>
__device__ __forceinline__ void rank_net_merge(uint32_t (&key)[P])
{
    if constexpr (J >= 1) {
        rank_net_step<P, K2, J, J == K2 / 2>(key);
        rank_net_merge<P, K2, J / 2>(key);
    }
}

template <int P, int K2 = 2>
__device__ __forceinline__ void rank_net_sort(uint32_t (&key)[P])
{
    if constexpr (K2 <= P) {
        rank_net_merge<P, K2, K2 / 2>(key);
        rank_net_sort<P, K2 * 2>(key);
    }
}

template <int P>
__global__ __launch_bounds__(256) void rank_finish_reg_kernel(size_t base, const uint32_t *__restrict__ keys, const RankFinish a)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.window) return;
    uint32_t key[P];
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < P; i++) {
        // planes at and past a.n read the last plane and are padded over: scalar arithmetic, no lane mask per register
        const uint32_t plane = (uint32_t)i < a.n ? (uint32_t)i : a.n - 1u;
        const uint32_t pad = (uint32_t)((int32_t)(a.n - 1u - (uint32_t)i) >> 31);
        key[i] = keys[(size_t)plane * a.window + w] | pad;
        k += key[i] != RANK_SENTINEL;
    }
    if (a.count) a.count[w] = (uint16_t)k;
    if (!a.sort) return;
    if (k < a.min_count) {
        for (uint32_t j = 0; j < a.n_q; j++) a.quantiles[(size_t)j * a.window + w] = a.fill;
        if (a.mad) a.mad[w] = 0.0f;
        return;
    }
    auto get = [&](uint32_t lo, uint32_t hi, uint32_t &key_lo, uint32_t &key_hi) {
        key_lo = key_hi = 0;
        // lo and hi are known before the sort: tie them to its last step, or 2 P compare masks are formed ahead of it and
        // held in scalar registers across it
        asm volatile("" : "+v"(lo), "+v"(hi), "+v"(key[0]));
#pragma unroll
        for (int i = 0; i < P; i++) {
            key_lo = lo == (uint32_t)i ? key[i] : key_lo;
            key_hi = hi == (uint32_t)i ? key[i] : key_hi;
        }
    };
    // two passes over one copy of the network: the values, then their distances from the median
#pragma nounroll
    for (int pass = 0; pass < 2; pass++) {
        rank_net_sort<P>(key);
        if (pass == 1) {
            a.mad[w] = rank_quantile<true>(0.5, k, get);
            return;
        }
        for (uint32_t j = 0; j < a.n_q; j++) a.quantiles[(size_t)j * a.window + w] = rank_quantile<false>(a.q[j], k, get);
        if (!a.mad) return;
        const float m = rank_quantile<false>(0.5, k, get);
        if (!(m - m == 0.0f)) {                             // not finite
            a.mad[w] = __uint_as_float(0x7FC00000u);
            return;
        }
#pragma unroll
        for (int i = 0; i < P; i++) key[i] = key[i] != RANK_SENTINEL ? rank_distance(key[i], m) : RANK_SENTINEL;
    }
}

// ---- tier 2: the keys of a tile of voxels in LDS --------------------------------------------------------------------------

// the whole network over the T segments of P keys in s (key n of voxel t at n * T + t): T * P / 2 exchanges per step, spread
// over the block's 256 threads; a barrier closes every step
template <int P>
__device__ __forceinline__ void rank_lds_sort(uint32_t *s)
{
    constexpr uint32_t T = RANK_LDS_KEYS / P;
    for (uint32_t k2 = 2; k2 <= (uint32_t)P; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j >= 1; j >>= 1) {
            const bool first = j == k2 >> 1;
            for (uint32_t e = threadIdx.x; e < RANK_LDS_KEYS / 2; e += 256) {
                const uint32_t t = e % T, p = e / T;
                const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));
                const uint32_t l = first ? (i ^ (k2 - 1u)) : (i | j);
                const uint32_t x = s[i * T + t], y = s[l * T + t];
                if (x > y) { s[i * T + t] = y; s[l * T + t] = x; }
            }
            __syncthreads();
        }
    }
}

// one block per tile; blockIdx counts tiles from base / 256 (the launch's work-items are the tiles padded to whole blocks)
template <int P>
__global__ __launch_bounds__(256) void rank_finish_lds_kernel(size_t base, const uint32_t *__restrict__ keys, const RankFinish a)
{
    constexpr uint32_t T = RANK_LDS_KEYS / P;
    __shared__ uint32_t s[RANK_LDS_KEYS];
    __shared__ float s_m[T];
    const size_t v0 = (base / 256 + blockIdx.x) * T;
    for (uint32_t e = threadIdx.x; e < RANK_LDS_KEYS; e += 256) {
        const uint32_t t = e % T, i = e / T;
        const size_t w = v0 + t;
        s[e] = i < a.n && w < a.window ? keys[(size_t)i * a.window + w] : RANK_SENTINEL;
    }
    __syncthreads();
    if (a.sort) rank_lds_sort<P>(s);
    const uint32_t t = threadIdx.x;
    const size_t w = v0 + t;
    const bool mine = t < T && w < a.window;
    auto get = [&](uint32_t lo, uint32_t hi, uint32_t &key_lo, uint32_t &key_hi) {
        key_lo = s[lo * T + t];
        key_hi = s[hi * T + t];
    };
    uint32_t k = 0;
    bool enough = false;
    if (mine) {
        if (a.sort) {
            // sorted: k is the position of the first sentinel
            uint32_t lo = 0, hi = P;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s[mid * T + t] != RANK_SENTINEL) lo = mid + 1; else hi = mid;
            }
            k = lo;
        } else {
            for (uint32_t i = 0; i < a.n; i++) k += s[i * T + t] != RANK_SENTINEL;
        }
        if (a.count) a.count[w] = (uint16_t)k;
        enough = k >= a.min_count;
        if (a.sort && !enough) {
            for (uint32_t j = 0; j < a.n_q; j++) a.quantiles[(size_t)j * a.window + w] = a.fill;
            if (a.mad) a.mad[w] = 0.0f;
        }
        if (a.sort && enough) {
            for (uint32_t j = 0; j < a.n_q; j++) a.quantiles[(size_t)j * a.window + w] = rank_quantile<false>(a.q[j], k, get);
            if (a.mad) s_m[t] = rank_quantile<false>(0.5, k, get);
        }
    }
    if (!a.sort || !a.mad) return;
    if (t < T && !(mine && enough)) s_m[t] = 0.0f;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < RANK_LDS_KEYS; e += 256) {
        const uint32_t key = s[e];
        if (key != RANK_SENTINEL) s[e] = rank_distance(key, s_m[e % T]);
    }
    __syncthreads();
    rank_lds_sort<P>(s);
    if (mine && enough) {
        const float m = s_m[t];
        a.mad[w] = m - m == 0.0f ? rank_quantile<true>(0.5, k, get) : __uint_as_float(0x7FC00000u);
    }
}
