// k_glm.hip.h -- a per-voxel linear model over the images of a group and its permutation test (frog_glm, include/frog_chain.h,
// which states the arithmetic line by line): the collect kernels, which store one f32 per voxel and add, the kernel that lays
// out the design rows of a batch of permutations, and the fit kernel that finish and permute share.
// Included by chain.hip inside its anonymous namespace, after the reslice, cover and rank device code it reuses.
//
// Fit.  One thread per voxel and a block per TILE of GLM_TILE consecutive window voxels, which it walks 256 at a time.  For
// each 256 voxels the block reads the n values of every voxel once and then loops over the permutations of the launch, so a
// permutation costs no HBM traffic: up to GLM_LDS_MAX images the values sit in LDS (value i of thread t at word i * 256 + t: a
// thread reads only its own column, conflict-free, and no barrier is needed), above it they are re-read through the caches.
// The design rows X' of permutation k do not depend on the voxel: glm_table_kernel writes, per permutation and image, the p
// entries of X'_i and the p (p + 1) / 2 products X'_ir * X'_ic -- each the one rounded multiplication the header states -- and
// the fit kernel reads them with wave-uniform addresses.  So a thread's normal equations cost one addition per entry.
// An image that does not take part at a voxel adds +0.0 to every sum (its product is replaced by +0.0, its value by +0.0
// before the multiplication): no sum here is ever -0.0, so x + (+-0.0) is x and the sums carry the bits of the loop over the
// participating set alone, with the same trip count in every lane.
// P, the number of columns, is a template argument: the packed lower triangle A (which L overwrites in place), b, D and beta
// live in registers under compile-time indices.
//
// Extrema.  t as a float maps to rank_key's u32, whose unsigned order is the order of the floats; the maximum and minimum of
// keys are exact and do not depend on the order they are taken in.  Per permutation and contrast: a wave's reduction by
// DPP moves, one LDS atomic per wave, and at the end of the tile one integer global atomic per block.  No floating-point
// atomic anywhere.
//
// Sink.  frog_glm_permute_clusters instantiates the fit kernel with a GlmSink: the voxels that count towards an extremum and
// lie beyond the cluster-forming threshold get their bit set in the masks of a frog_clusters (k_ccl.hip.h), a ballot per
// wavefront, contrast and side and an integer atomicOr where it is not zero.  Without one the kernel is what it was.
#pragma once

constexpr uint32_t GLM_NAN_BITS = 0x7FC00000u;
constexpr uint32_t GLM_LDS_MAX = 48;                // the largest n_images whose values a block keeps in LDS (48 KiB)
constexpr uint32_t GLM_TILE = 2048;                 // window voxels of a block: 8 per thread
constexpr uint32_t GLM_BATCH = 64;                  // the most permutations of one launch
constexpr size_t GLM_TABLE_BYTES = (size_t)32 << 20;        // the design rows of one launch's permutations stay below this
constexpr uint32_t GLM_KEY_NEG_INF = 0x007FFFFFu;   // rank_key(-inf): where a maximum starts
constexpr uint32_t GLM_KEY_POS_INF = 0xFF800000u;   // rank_key(+inf): where a minimum starts

static_assert(FROG_GLM_MAX_COLUMNS == 8 && FROG_GLM_MAX_CONTRASTS == 8, "the fit kernel is instantiated for 1 to 8 columns");

// what an add stores for a voxel: x where the voxel is valid and x is finite, the quiet NaN elsewhere
__device__ __forceinline__ float glm_entry(bool valid, float x)
{
    return valid && x - x == 0.0f ? x : __uint_as_float(GLM_NAN_BITS);
}

// window_reslice_kernel and window_identity_kernel (k_rank.hip.h) with the float store
struct GlmEntry {
    using type = float;
    static __device__ __forceinline__ type of(bool valid, float x) { return glm_entry(valid, x); }
};

// The determinant chain_sample_kernel stores for the node (grid_node, chain_point<true>, det3), and the validity of
// cover_reslice_kernel at the position the same evaluation of the chain gives: inside `support` (where there is one), then
// the mask.  log_mode: (float)log(det) where det > 0, no entry elsewhere.
__global__ __launch_bounds__(256) void glm_jacobian_kernel(size_t base, size_t first, size_t window, const DevLink *links, int n_links,
                                                           const NodeGrid out, int has_support, const MaskGrid support,
                                                           const uint8_t *__restrict__ mask, const MaskGrid mg, int log_mode,
                                                           float *__restrict__ plane)
{
    const size_t w = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= window) return;
    const size_t idx = first + w;
    double p[3], c[3], A[3][3];
    grid_node(out, idx, p);
    chain_point<true>(links, n_links, p, A);
    const double det = det3(A);
    bool valid = !has_support || voxel_coordinates(p, support.so, support.ss, support.sx, support.sy, support.sz, c);
    if (valid && mask) valid = mask_covers(p, mask, mg);
    float x;
    if (log_mode) {
        valid = valid && det > 0.0;
        x = valid ? (float)log(det) : 0.0f;
    } else {
        x = (float)det;
    }
    plane[w] = glm_entry(valid, x);
}

__host__ __device__ constexpr int glm_tri(int r, int c) { return r * (r + 1) / 2 + c; }
__host__ __device__ constexpr size_t glm_row_doubles(uint32_t p) { return (size_t)p + (size_t)p * (p + 1) / 2; }

// Row (k, i) of the table of a launch's permutations k < n_perms: X'_i0 .. X'_i(p-1), then the products of the lower
// triangle, row by row.  perm and sign null: the design as it is (finish).
__global__ __launch_bounds__(256) void glm_table_kernel(size_t base, const double *__restrict__ design, const uint32_t *__restrict__ perm,
                                                        const int8_t *__restrict__ sign, uint32_t n, uint32_t p, uint32_t columns,
                                                        size_t total, double *__restrict__ table)
{
    const size_t e = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint32_t i = (uint32_t)(e % n);
    const uint32_t from = perm ? perm[e] : i;
    const double s = sign ? (double)sign[e] : 1.0;
    double *row = table + e * glm_row_doubles(p);
    double x[FROG_GLM_MAX_COLUMNS];
    for (uint32_t j = 0; j < p; j++) {
        const double moved = s * design[(size_t)from * p + j];
        x[j] = ((columns >> j) & 1u) ? moved : design[(size_t)i * p + j];
        row[j] = x[j];
    }
    for (uint32_t r = 0; r < p; r++)
        for (uint32_t c = 0; c <= r; c++) row[p + glm_tri((int)r, (int)c)] = x[r] * x[c];
}

// what a launch of the fit kernel takes by value beside the values and the table
struct GlmArgs {
    size_t window, tiles;
    uint32_t n;                     // images
    uint32_t need;                  // max(min_count, p + 1)
    uint32_t n_contrasts, n_perms;  // n_perms: the permutations of this launch
    double sigma_floor;
    float fill;
    double contrasts[FROG_GLM_MAX_CONTRASTS * FROG_GLM_MAX_COLUMNS];       // contrast c at [c * p, c * p + p)
    const uint8_t *region;          // window-sized, or null
    float *beta, *sigma, *t;        // finish's outputs; any may be null
    uint16_t *count;
    uint32_t *extrema;              // permute: per permutation and contrast the keys of the maximum and of the minimum; or null
};


// An image that does not take part adds +0.0: its terms are ANDed with zero bits, the others with ones.  A select would do, but
// the compiler turns a select of a wave-uniform load into a branch around the load, one scalar round trip per term; the AND
// keeps the row's loads together ahead of the arithmetic.
__device__ __forceinline__ uint64_t glm_keep(float f) { return f == f ? ~(uint64_t)0 : (uint64_t)0; }
__device__ __forceinline__ double glm_masked(double v, uint64_t keep)
{
    return __longlong_as_double((long long)((uint64_t)__double_as_longlong(v) & keep));
}

// One voxel under one permutation, as the header states it.  value(i) is the stored f32 of image i at the voxel, rows the
// table rows of the permutation, k the voxel's participating images.  Returns whether the voxel is fit (the pivot test);
// beta, sd and, through store(c, t), the contrasts' t are meaningful only then.
template <int P, class Value, class Store>
__device__ __forceinline__ bool glm_voxel(const GlmArgs &a, const double *__restrict__ rows, uint32_t k, Value value, double (&beta)[P],
                                          double &sd, Store store)
{
    constexpr int TRI = P * (P + 1) / 2, ROW = P + TRI;
    double A[TRI], D[P];
#pragma unroll
    for (int e = 0; e < TRI; e++) A[e] = 0.0;
#pragma unroll
    for (int r = 0; r < P; r++) beta[r] = 0.0;                      // b, then in place z, y and beta
    for (uint32_t i = 0; i < a.n; i++) {
        const double *const row = rows + (size_t)i * ROW;
        const float f = value(i);
        const uint64_t keep = glm_keep(f);
        const double y = glm_masked((double)f, keep);
        if (__all(f == f)) {                                        // the whole wavefront takes image i: the products as loaded
#pragma unroll
            for (int e = 0; e < TRI; e++) A[e] = A[e] + row[P + e];
        } else {
#pragma unroll
            for (int e = 0; e < TRI; e++) {
                const double m = glm_masked(row[P + e], keep);
                A[e] = A[e] + m;
            }
        }
#pragma unroll
        for (int r = 0; r < P; r++) {
            const double m = row[r] * y;
            beta[r] = beta[r] + m;
        }
    }
    // LDL^T in place: L_ij takes A_ij's place below the diagonal; the diagonal keeps A_jj for the pivot test
    bool fit = true;
#pragma unroll
    for (int j = 0; j < P; j++) {
        const double ajj = A[glm_tri(j, j)];
        double dj = ajj;
#pragma unroll
        for (int q = 0; q < j; q++) {
            const double l = A[glm_tri(j, q)];
            const double sq = l * l;
            const double m = sq * D[q];
            dj = dj - m;
        }
        D[j] = dj;
        const double limit = 0x1p-40 * ajj;
        fit = fit && ajj > 0.0 && dj > limit;
#pragma unroll
        for (int i = j + 1; i < P; i++) {
            double x = A[glm_tri(i, j)];
#pragma unroll
            for (int q = 0; q < j; q++) {
                const double lq = A[glm_tri(i, q)] * A[glm_tri(j, q)];
                const double m = lq * D[q];
                x = x - m;
            }
            A[glm_tri(i, j)] = x / dj;
        }
    }
    // A z = rhs with the factor, in place: forward, diagonal, backward
    auto solve = [&](double (&z)[P]) {
#pragma unroll
        for (int i = 0; i < P; i++) {
#pragma unroll
            for (int q = 0; q < i; q++) {
                const double m = A[glm_tri(i, q)] * z[q];
                z[i] = z[i] - m;
            }
        }
#pragma unroll
        for (int i = 0; i < P; i++) z[i] = z[i] / D[i];
#pragma unroll
        for (int i = P - 1; i >= 0; i--) {
#pragma unroll
            for (int q = i + 1; q < P; q++) {
                const double m = A[glm_tri(q, i)] * z[q];
                z[i] = z[i] - m;
            }
        }
    };
    solve(beta);
    double rss = 0.0;
#pragma unroll 4
    for (uint32_t i = 0; i < a.n; i++) {
        const double *const row = rows + (size_t)i * ROW;
        const float f = value(i);
        const uint64_t keep = glm_keep(f);
        const double y = glm_masked((double)f, keep);
        double fitted = 0.0;
#pragma unroll
        for (int j = 0; j < P; j++) {
            const double m = row[j] * beta[j];
            fitted = fitted + m;
        }
        const double r = y - fitted;
        const double q = r * r;
        rss = rss + glm_masked(q, keep);
    }
    const double s2 = rss / (double)(k - (uint32_t)P);
    sd = sqrt(s2);
    for (uint32_t c = 0; c < a.n_contrasts; c++) {
        const double *const con = a.contrasts + c * P;
        double u[P];
#pragma unroll
        for (int j = 0; j < P; j++) u[j] = con[j];
        solve(u);
        double v = 0.0, e = 0.0;
#pragma unroll
        for (int j = 0; j < P; j++) {
            const double m = con[j] * u[j];
            v = v + m;
        }
#pragma unroll
        for (int j = 0; j < P; j++) {
            const double m = con[j] * beta[j];
            e = e + m;
        }
        double den = s2 * v;
        den = sqrt(den);
        const double ratio = e / den;
        float t = (float)ratio;
        if (sd <= a.sigma_floor || !(t - t == 0.0f)) t = __uint_as_float(GLM_NAN_BITS);
        store(c, t);
    }
    return fit;
}

// The largest (MAX) or smallest of v over the wavefront, in lane 63.  Within each row of 16 lanes row_shr 1, 2, 4 and 8 leave the
// row's extreme in its last lane; row_bcast 15 then carries it into rows 1 and 3, row_bcast 31 the first half's into the
// second.  A lane without a source keeps its own value, which an extreme absorbs.  Every lane of the wavefront must be active.
template <bool MAX>
__device__ __forceinline__ uint32_t glm_wave_extreme(uint32_t v)
{
#define GLM_DPP_STEP(ctrl, rows)                                                                                   \
    {                                                                                                              \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rows, 0xf, false);          \
        v = MAX ? max(v, o) : min(v, o);                                                                           \
    }
    GLM_DPP_STEP(0x111, 0xf)
    GLM_DPP_STEP(0x112, 0xf)
    GLM_DPP_STEP(0x114, 0xf)
    GLM_DPP_STEP(0x118, 0xf)
    GLM_DPP_STEP(0x142, 0xa)
    GLM_DPP_STEP(0x143, 0xc)
#undef GLM_DPP_STEP
    return v;
}

// where glm_fit_kernel sets the bits of the supra-threshold voxels: the masks of a frog_clusters (k_ccl.hip.h states
// their layout), slot (permutation, contrast, side) at bits + slot * words
struct GlmSink {
    uint32_t *bits;
    size_t words;
    size_t first;                                   // the window's first voxel in the grid
    uint32_t perm0;                                 // the sink's permutation of the launch's first
    uint32_t sides;
    float threshold;
};
__device__ __forceinline__ const GlmSink &glm_the_sink(const GlmSink &sink) { return sink; }

// where glm_fit_kernel stores the levels of the voxels: the level maps of a frog_tfce (k_tfce.hip.h states their layout and
// the level of a statistic, glm_level below restates it), slot (permutation, contrast, side) at levels + slot * stride
struct GlmLevelSink {
    uint8_t *levels;
    size_t stride;
    size_t first;                                   // the window's first voxel in the grid
    uint32_t perm0;                                 // the sink's permutation of the launch's first
    uint32_t sides;
    float dh;
};
__device__ __forceinline__ const GlmLevelSink &glm_the_sink(const GlmLevelSink &sink) { return sink; }

// trunc(s / dh) saturated at 255 for s = t (side 0) or -t (side 1), 0 where s is not positive: one f64 division
__device__ __forceinline__ uint8_t glm_level(float t, uint32_t side, float dh)
{
    const float s = side ? -t : t;
    if (!(s > 0.0f)) return 0;
    const double q = (double)s / (double)dh;
    return q >= 255.0 ? (uint8_t)255 : (uint8_t)q;
}

// The bits of the wavefront's 64 consecutive voxels, the first at grid index g0, into `mask`: the ballot shifted to g0's place
// in its word spans up to three words, which lanes 0 to 2 OR in where they are not zero.  A word past the mask's end would
// hold bits of voxels past the grid's, which are never on.  Every lane of the wavefront must be active.
__device__ __forceinline__ void glm_sink_store(uint32_t *mask, size_t g0, bool on)
{
    const unsigned long long m = __ballot(on);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u, shift = (uint32_t)(g0 & 31u);
    const unsigned long long low = m << shift;
    const uint32_t word = lane == 0u ? (uint32_t)low : lane == 1u ? (uint32_t)(low >> 32) : (shift ? (uint32_t)(m >> (64u - shift)) : 0u);
    if (lane < 3u && word) atomicOr(mask + (g0 >> 5) + lane, word);
}

// One block per tile; blockIdx counts tiles from base / 256 (the launch's work-items are the tiles padded to whole blocks).
// Dynamic LDS: 2 n_perms n_contrasts keys where extrema are wanted, then with LDS 256 n floats.
// Sink is empty (finish and frog_glm_permute: the kernel takes no further argument) or one GlmSink (frog_glm_permute_clusters),
// with which the kernel also sets the bit of every voxel that counts towards an extremum and lies beyond the threshold, in the
// sink's mask of its permutation, contrast and side, at the voxel's index in the whole grid; or one GlmLevelSink
// (frog_glm_permute_tfce), with which it stores there, one byte per voxel, that voxel's level on each side instead.
template <int P, bool LDS, class... Sink>
__global__ __launch_bounds__(256) void glm_fit_kernel(size_t base, const float *__restrict__ vals, const double *__restrict__ table, const GlmArgs a,
                                                      const Sink... sink)
{
    extern __shared__ uint32_t glm_mem[];
    constexpr int ROW = P + P * (P + 1) / 2;
    const size_t tile = base / 256 + blockIdx.x;            // the same for every thread of the block
    if (tile >= a.tiles) return;
    const uint32_t tid = threadIdx.x, C = a.n_contrasts, n_ext = a.extrema ? a.n_perms * C * 2u : 0u;
    uint32_t *const ext = glm_mem;
    float *const ys = (float *)(glm_mem + n_ext) + tid;
    for (uint32_t e = tid; e < n_ext; e += 256) ext[e] = (e & 1u) ? GLM_KEY_POS_INF : GLM_KEY_NEG_INF;
    __syncthreads();

    for (uint32_t s = 0; s < GLM_TILE / 256; s++) {
        const size_t w0 = tile * GLM_TILE + (size_t)s * 256;
        if (w0 >= a.window) break;
        const size_t w = w0 + tid;
        const bool live = w < a.window;
        uint32_t k = 0;
        for (uint32_t i = 0; i < a.n; i++) {
            const float f = live ? vals[(size_t)i * a.window + w] : __uint_as_float(GLM_NAN_BITS);
            if (LDS) ys[i * 256u] = f;
            k += f == f;
        }
        if (a.count && live) a.count[w] = (uint16_t)k;
        const bool wanted = live && k >= a.need && (!a.region || a.region[w] != 0);
        auto value = [&](uint32_t i) -> float { return LDS ? ys[i * 256u] : vals[(size_t)i * a.window + w]; };

        if (!a.extrema) {
            // finish: the design as it is, every output
            if (!live) continue;
            double beta[P], sd = 0.0;
            bool fit = false;
            if (wanted)
                fit = glm_voxel<P>(a, table, k, value, beta, sd, [&](uint32_t c, float t) { if (a.t) a.t[(size_t)c * a.window + w] = t; });
            if (a.beta)
                for (int j = 0; j < P; j++) a.beta[(size_t)j * a.window + w] = fit ? (float)beta[j] : a.fill;
            if (a.sigma) a.sigma[w] = fit ? (float)sd : a.fill;
            if (a.t && !fit)
                for (uint32_t c = 0; c < C; c++) a.t[(size_t)c * a.window + w] = a.fill;
            continue;
        }

        if (!__any(wanted)) continue;
        for (uint32_t kk = 0; kk < a.n_perms; kk++) {
            float ts[FROG_GLM_MAX_CONTRASTS] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            bool fit = false;
            if (wanted) {
                double beta[P], sd;
                fit = glm_voxel<P>(a, table + (size_t)kk * a.n * ROW, k, value, beta, sd, [&](uint32_t c, float t) {
#pragma unroll
                    for (uint32_t j = 0; j < FROG_GLM_MAX_CONTRASTS; j++) ts[j] = j == c ? t : ts[j];
                });
            }
            for (uint32_t c = 0; c < C; c++) {
                float t = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < FROG_GLM_MAX_CONTRASTS; j++) t = j == c ? ts[j] : t;
                const bool counts = fit && t == t;
                const uint32_t hi = glm_wave_extreme<true>(counts ? rank_key(t) : GLM_KEY_NEG_INF);
                const uint32_t lo = glm_wave_extreme<false>(counts ? rank_key(t) : GLM_KEY_POS_INF);
                if ((tid & 63u) == 63u) {
                    atomicMax(&ext[(kk * C + c) * 2u], hi);
                    atomicMin(&ext[(kk * C + c) * 2u + 1u], lo);
                }
                if constexpr ((std::is_same_v<Sink, GlmSink> || ...)) {
                    // f32 comparisons on the t the extrema are taken over; side 0 above the threshold, side 1 below its negative
                    const GlmSink &to = glm_the_sink(sink...);
                    uint32_t *const mask = to.bits + ((size_t)(to.perm0 + kk) * C + c) * to.sides * to.words;
                    const size_t g0 = to.first + w0 + (tid & ~63u);
                    glm_sink_store(mask, g0, counts && t > to.threshold);
                    if (to.sides == 2u) glm_sink_store(mask + to.words, g0, counts && t < -to.threshold);
                }
                if constexpr ((std::is_same_v<Sink, GlmLevelSink> || ...)) {
                    // every window voxel's own byte: its level where it counts, 0 where it does not
                    const GlmLevelSink &to = glm_the_sink(sink...);
                    uint8_t *const level = to.levels + ((size_t)(to.perm0 + kk) * C + c) * to.sides * to.stride + to.first + w;
                    if (live) {
                        level[0] = counts ? glm_level(t, 0u, to.dh) : (uint8_t)0;
                        if (to.sides == 2u) level[to.stride] = counts ? glm_level(t, 1u, to.dh) : (uint8_t)0;
                    }
                }
            }
        }
    }
    if (!n_ext) return;
    __syncthreads();
    for (uint32_t e = tid; e < n_ext; e += 256) {
        if (e & 1u) atomicMin(&a.extrema[e], ext[e]);
        else atomicMax(&a.extrema[e], ext[e]);
    }
}
