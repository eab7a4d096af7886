// k_staple.hip.h -- multi-label STAPLE over the label maps of a group (frog_staple, include/frog_chain.h, which states the
// arithmetic line by line): the kernels of an add, of finish and of one EM iteration, and the getters'.
// Included by chain.hip inside its anonymous namespace, after the label map (LabelMap, label_find) it reuses.
//
// Data.  D[i][v], one byte: the dense index of image i's label at voxel v, plane i at D + i * V.  q[l][v], u32 in units of
// 2^-30: plane l at q + l * V, stored (not recomputed), so the M-step, the getters and a later solve read what the E-step
// wrote.  theta[i][l'][l], S[i][l'][l]: entry (i * L + l') * L + l, so the row an image's label selects is L contiguous
// words.  Every index above is formed in size_t: i * V and l * V pass 2^32 long before the grid's 2^31 voxels do.
//
// E-step.  One thread per active voxel, the (m, e) of a tile of LT labels in registers (every index a compile-time
// constant).  Up to STAPLE_TILE_MAX labels are one tile; above that the voxel is swept three times over the tiles in
// ascending order -- emax, then s, then q -- recomputing the products, which are the same bits every time because each is
// the same sequence of rounded operations.  Neighbouring voxels nearly always carry the same label, so a wave reads one row
// of theta per image.
//
// M-step.  S has n * L * L u64 words fed by A * n * L contributions; integer sums, so any order is exact.  A block owns one
// tile of S -- IT images x L shown labels x LW true labels, at most STAPLE_ACC_WORDS words of LDS -- and a share of the
// voxels, which it strides over in chunks of 256.  Per chunk a wave first reduces sum over its lanes of q[l][.] for the LW
// labels with a butterfly of shuffles, after which lane l keeps the sum of label l.  Then per image of the tile: where all
// the wave's active lanes carry one label (found with a ballot; the common case) lanes 0 .. LW-1 add their wave sums to
// S[i][that label][.], LW LDS atomics to LW addresses; only a mixed wave takes the per-lane path, one LDS atomic per lane
// and label.  At the end the block flushes its non-zero words with 64-bit global atomics.  T[l] is the column sum of
// S[0][.][l]: every active voxel has exactly one D[0][v].
#pragma once

constexpr double STAPLE_FLOOR = 0x1p-24;
constexpr uint32_t STAPLE_ONE = 1u << 30;
constexpr uint32_t STAPLE_K = 16;                   // factors between two renormalisations
constexpr uint32_t STAPLE_TILE_MAX = 32;            // labels a thread of the E-step keeps in registers
constexpr uint32_t STAPLE_ACC_WORDS = 6144;         // u64 accumulators of an M-step block: 48 KiB of LDS
constexpr uint32_t STAPLE_MSTEP_BLOCKS = 1024;      // persistent blocks of an M-step, over all its tiles

static_assert(FROG_STAPLE_MAX_LABELS == 256, "D holds one byte per image and voxel");
static_assert(STAPLE_ACC_WORDS >= FROG_STAPLE_MAX_LABELS, "a tile holds at least one true label of one image");

// phase 2 of an add: the voxel's dense index (in the order of the inserts; finish renumbers) into the image's plane
template <class S>
__global__ __launch_bounds__(256) void staple_index_kernel(size_t base, const S *__restrict__ labels, size_t total, const LabelMap m,
                                                           uint8_t *__restrict__ plane)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    plane[idx] = (uint8_t)label_find(m, (long long)labels[idx]);
}

struct StapleLut { uint8_t to[FROG_STAPLE_MAX_LABELS]; };

// finish: dense index -> position of its value in ascending order, over all n * V bytes of D
__global__ __launch_bounds__(256) void staple_renumber_kernel(size_t base, uint8_t *__restrict__ D, size_t count, const StapleLut lut)
{
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count) return;
    D[idx] = lut.to[D[idx]];
}

// The opening of a solve, one thread per voxel: whether the voxel is active, c[l] over the active voxels, and the q of an
// inactive voxel.  The thread counts runs of equal labels along the images, so a unanimous voxel costs one LDS atomic.
__global__ __launch_bounds__(256) void staple_active_kernel(size_t base, const uint8_t *__restrict__ D, size_t V, uint32_t n, uint32_t L,
                                                            int restrict_to_disputed, uint8_t *__restrict__ active,
                                                            uint32_t *__restrict__ q, unsigned long long *__restrict__ c)
{
    __shared__ uint32_t hist[FROG_STAPLE_MAX_LABELS];          // at most 256 threads x 4096 images
    hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) {
        const uint32_t first = D[v];
        bool unanimous = true;
        for (uint32_t i = 1; i < n && unanimous; i++) unanimous = D[(size_t)i * V + v] == first;
        const bool is_active = !restrict_to_disputed || !unanimous;
        active[v] = is_active;
        if (!is_active) {
            for (uint32_t l = 0; l < L; l++) q[(size_t)l * V + v] = l == first ? STAPLE_ONE : 0u;
        } else if (unanimous) {
            atomicAdd(&hist[first], n);
        } else {
            uint32_t run = first, length = 1;
            for (uint32_t i = 1; i < n; i++) {
                const uint32_t d = D[(size_t)i * V + v];
                if (d == run) { length++; continue; }
                atomicAdd(&hist[run], length);
                run = d; length = 1;
            }
            atomicAdd(&hist[run], length);
        }
    }
    __syncthreads();
    if (threadIdx.x < L && hist[threadIdx.x]) atomicAdd(&c[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// (m, e) of labels l0 .. l0 + LT - 1 at voxel v: lines 1 to 3 of the E-step.  A label past L has m = 0.
template <int LT>
__device__ __forceinline__ void staple_products(const uint8_t *__restrict__ D, size_t V, size_t v, uint32_t n, uint32_t L, uint32_t l0,
                                                const double *__restrict__ theta, const double *__restrict__ prior, double (&m)[LT],
                                                int (&e)[LT])
{
#pragma unroll
    for (int j = 0; j < LT; j++) { m[j] = l0 + j < L ? prior[l0 + j] : 0.0; e[j] = 0; }
    for (uint32_t i = 0; i < n; i++) {
        const double *__restrict__ row = theta + ((size_t)i * L + D[(size_t)i * V + v]) * L + l0;
#pragma unroll
        for (int j = 0; j < LT; j++)
            if (l0 + j < L) m[j] = m[j] * fmax(row[j], STAPLE_FLOOR);
        if (i % STAPLE_K == STAPLE_K - 1 || i == n - 1) {
#pragma unroll
            for (int j = 0; j < LT; j++) { int k; m[j] = frexp(m[j], &k); e[j] += k; }
        }
    }
}

template <int LT>
__global__ __launch_bounds__(256) void staple_estep_kernel(size_t base, const uint8_t *__restrict__ D, size_t V, uint32_t n, uint32_t L,
                                                           const double *__restrict__ theta, const double *__restrict__ prior,
                                                           const uint8_t *__restrict__ active, uint32_t *__restrict__ q)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V || !active[v]) return;
    double m[LT];
    int e[LT];
    int emax = std::numeric_limits<int>::min();
    double s = 0.0;
    if (L <= (uint32_t)LT) {                            // one tile: nothing is computed twice
        staple_products<LT>(D, V, v, n, L, 0, theta, prior, m, e);
#pragma unroll
        for (int j = 0; j < LT; j++) if (m[j] > 0.0 && e[j] > emax) emax = e[j];
#pragma unroll
        for (int j = 0; j < LT; j++) { m[j] = ldexp(m[j], e[j] - emax); s = s + m[j]; }
#pragma unroll
        for (int j = 0; j < LT; j++)
            if ((uint32_t)j < L) q[(size_t)j * V + v] = (uint32_t)rint((m[j] / s) * (double)STAPLE_ONE);
        return;
    }
    for (uint32_t l0 = 0; l0 < L; l0 += LT) {
        staple_products<LT>(D, V, v, n, L, l0, theta, prior, m, e);
#pragma unroll
        for (int j = 0; j < LT; j++) if (m[j] > 0.0 && e[j] > emax) emax = e[j];
    }
    for (uint32_t l0 = 0; l0 < L; l0 += LT) {
        staple_products<LT>(D, V, v, n, L, l0, theta, prior, m, e);
#pragma unroll
        for (int j = 0; j < LT; j++) s = s + ldexp(m[j], e[j] - emax);          // a label past L adds +0.0
    }
    for (uint32_t l0 = 0; l0 < L; l0 += LT) {
        staple_products<LT>(D, V, v, n, L, l0, theta, prior, m, e);
#pragma unroll
        for (int j = 0; j < LT; j++)
            if (l0 + j < L) q[(size_t)(l0 + j) * V + v] = (uint32_t)rint((ldexp(m[j], e[j] - emax) / s) * (double)STAPLE_ONE);
    }
}

// How the M-step cuts S into the tiles of its blocks (see the head of this file).
struct StapleTiles {
    uint32_t n, L;
    uint32_t lw, it;                // true labels and images of a tile
    uint32_t label_tiles, tiles;    // tiles along l; all tiles
    uint32_t per_tile;              // blocks that share a tile's voxels
    size_t chunks;                  // chunks of 256 voxels
};

__host__ inline StapleTiles staple_tiles(uint32_t n, uint32_t L, size_t V)
{
    StapleTiles t;
    t.n = n; t.L = L;
    t.lw = std::min(std::min(L, 64u), STAPLE_ACC_WORDS / L);
    t.it = std::max(1u, std::min(n, STAPLE_ACC_WORDS / (L * t.lw)));
    t.label_tiles = (L + t.lw - 1) / t.lw;
    t.tiles = ((n + t.it - 1) / t.it) * t.label_tiles;
    t.chunks = (V + 255) / 256;
    t.per_tile = (uint32_t)std::max<size_t>(1, std::min<size_t>(t.chunks, STAPLE_MSTEP_BLOCKS / t.tiles));
    return t;
}

// UNIFORM = false takes the per-lane path for every wave: the measurement's other arm, and the same sums.
template <bool UNIFORM>
__global__ __launch_bounds__(256) void staple_mstep_kernel(size_t base, const uint8_t *__restrict__ D, size_t V, const StapleTiles t,
                                                           const uint8_t *__restrict__ active, const uint32_t *__restrict__ q,
                                                           unsigned long long *__restrict__ S)
{
    __shared__ unsigned long long acc[STAPLE_ACC_WORDS];
    const size_t block = base / 256 + blockIdx.x;
    const uint32_t tile = (uint32_t)(block / t.per_tile), share = (uint32_t)(block % t.per_tile);
    if (tile >= t.tiles) return;                        // the block is uniform in this: no barrier is skipped by a part of it
    const uint32_t i0 = (tile / t.label_tiles) * t.it, l0 = (tile % t.label_tiles) * t.lw;
    const uint32_t ni = min(t.it, t.n - i0), nl = min(t.lw, t.L - l0), L = t.L;
    const uint32_t words = ni * L * nl;                 // acc[(ii * L + l') * nl + l]
    for (uint32_t w = threadIdx.x; w < words; w += 256) acc[w] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    for (size_t chunk = share; chunk < t.chunks; chunk += t.per_tile) {
        const size_t v = chunk * 256 + threadIdx.x;
        const bool valid = v < V && active[v];
        const unsigned long long lanes = __ballot(valid);
        if (!lanes) continue;                           // wave-uniform
        unsigned long long mine = 0;                    // lane l: the wave's sum of q[l0 + l][.]
        if (UNIFORM) {
            for (uint32_t l = 0; l < nl; l++) {
                unsigned long long x = valid ? q[(size_t)(l0 + l) * V + v] : 0u;
                for (int h = 32; h > 0; h >>= 1) x += __shfl_xor(x, h);
                if (lane == l) mine = x;
            }
        }
        const int leader = __ffsll((long long)lanes) - 1;
        for (uint32_t ii = 0; ii < ni; ii++) {
            const uint32_t d = valid ? D[(size_t)(i0 + ii) * V + v] : 0u;
            const uint32_t d0 = __shfl(d, leader);
            if (UNIFORM && !__ballot(valid && d != d0)) {
                if (lane < nl && mine) atomicAdd(&acc[(ii * L + d0) * nl + lane], mine);
            } else if (valid) {
                for (uint32_t l = 0; l < nl; l++) {
                    const uint32_t x = q[(size_t)(l0 + l) * V + v];
                    if (x) atomicAdd(&acc[(ii * L + d) * nl + l], (unsigned long long)x);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < words; w += 256) {
        const unsigned long long x = acc[w];
        if (!x) continue;
        const uint32_t l = w % nl, lp = (w / nl) % L, ii = w / (nl * L);
        atomicAdd(&S[((size_t)(i0 + ii) * L + lp) * L + l0 + l], x);
    }
}

// T[l] = sum over l' of S[0][l'][l], one thread per label
__global__ __launch_bounds__(256) void staple_totals_kernel(size_t base, const unsigned long long *__restrict__ S, uint32_t L,
                                                            unsigned long long *__restrict__ T)
{
    const size_t l = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    unsigned long long sum = 0;
    for (uint32_t lp = 0; lp < L; lp++) sum += S[(size_t)lp * L + l];
    T[l] = sum;
}

// theta from S and T, one thread per entry, and the largest |new - old|: the bits of a non-negative double order as its
// value does, so the maximum is an integer atomic and free of any order
__global__ __launch_bounds__(256) void staple_theta_kernel(size_t base, const unsigned long long *__restrict__ S,
                                                           const unsigned long long *__restrict__ T, uint32_t L, size_t count,
                                                           double *__restrict__ theta, unsigned long long *__restrict__ change)
{
    __shared__ unsigned long long s_max[4];
    const size_t idx = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bits = 0;
    if (idx < count) {
        const unsigned long long total = T[idx % L];
        if (total) {
            const double old = theta[idx], now = (double)S[idx] / (double)total;
            theta[idx] = now;
            bits = (unsigned long long)__double_as_longlong(fabs(now - old));
        }
    }
    for (int h = 32; h > 0; h >>= 1) { const unsigned long long o = __shfl_xor(bits, h); bits = o > bits ? o : bits; }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) bits = s_max[w] > bits ? s_max[w] : bits;
        if (bits) atomicMax(change, bits);
    }
}

// The first label in ascending order with the strictly largest q; confidence = (float)((double)q * 2^-30).
template <class T>
__global__ __launch_bounds__(256) void staple_fused_kernel(size_t base, const uint32_t *__restrict__ q, const long long *__restrict__ values,
                                                           uint32_t L, size_t V, T *__restrict__ label, float *__restrict__ confidence)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    uint32_t best = q[v], winner = 0;
    for (uint32_t l = 1; l < L; l++) {
        const uint32_t x = q[(size_t)l * V + v];
        if (x > best) { best = x; winner = l; }
    }
    if (label) label[v] = (T)values[winner];
    if (confidence) confidence[v] = (float)((double)best * 0x1p-30);
}

__global__ __launch_bounds__(256) void staple_probability_kernel(size_t base, const uint32_t *__restrict__ plane, size_t V, float *__restrict__ p)
{
    const size_t v = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    p[v] = (float)((double)plane[v] * 0x1p-30);
}
