// k_mesh.hip.h -- the kernels of frog_mesh_smooth, frog_isosurface_smooth and frog_isosurface_cluster (frog_chain.h): Taubin's
// lambda | mu filter on the vertex graph and decimation by vertex clustering.  Included by chain.hip inside its anonymous
// namespace, after k_iso.hip.h (chain.hip includes <hipcub/hipcub.hpp>).
//
// Smoothing.  The adjacency is built once per call:
//   mesh_edge_keys_kernel   both directed keys a << 32 | b of every face edge (a pair of equal indices: the sentinel n << 32 | n)
//   hipcub radix sort       the keys ascending: rows by vertex, columns ascending inside a row, the sentinels last
//   hipcub run lengths      the distinct keys and how often each occurs; once = a boundary edge
//   mesh_row_kernel         row offsets by binary search in the distinct keys
//   mesh_degree_kernel      |N(v)| by the header's rule (a boundary vertex keeps its boundary edges, or nothing)
//   mesh_fill_kernel        N(v) compacted behind the exclusive sum of the degrees: the CSR the passes read
// and then 2 x iterations launches of mesh_pass_kernel, one thread per vertex, positions ping-ponged between two buffers.
// No hashing and no atomics: every array is a function of the input alone.
//
// Clustering.  mesh_bounds_kernel + mesh_bounds_final_kernel (lo, hi, the count of non-finite values), mesh_cell_keys_kernel, a
// stable radix sort of (key, old index), run lengths, mesh_cluster_kernel (one thread per cluster: the f64 sums in ascending
// old index), mesh_triangle_count_kernel / mesh_triangle_emit_kernel (block scan + device scan, as iso_triangles_kernel).
#pragma once

constexpr int MESH_BLOCK = 256;
constexpr int MESH_BOUNDS_BLOCKS = 1024;        // partial results of the bounds reduction, at most

// ---- smoothing ------------------------------------------------------------------------------------------------------------------

// One thread per face; every index is below n (the entry points check the host arrays, frog_isosurface_create makes no other).  face_ptr == nullptr: triangles, face f holds idx[3 f .. 3 f + 3).  The edge that starts at slot j of
// face_idx writes keys[2 j] and keys[2 j + 1].
__global__ __launch_bounds__(MESH_BLOCK) void mesh_edge_keys_kernel(size_t base, const uint32_t *__restrict__ face_ptr,
                                                                    const uint32_t *__restrict__ face_idx, size_t n_faces, uint32_t n,
                                                                    unsigned long long *__restrict__ keys)
{
    const size_t f = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const size_t first = face_ptr ? (size_t)face_ptr[f] : 3 * f, last = face_ptr ? (size_t)face_ptr[f + 1] : 3 * f + 3;
    const unsigned long long none = (unsigned long long)n << 32 | n;
    for (size_t j = first; j < last; j++) {
        const unsigned long long a = face_idx[j], b = face_idx[j + 1 < last ? j + 1 : first];
        keys[2 * j] = a == b ? none : a << 32 | b;
        keys[2 * j + 1] = a == b ? none : b << 32 | a;
    }
}

// raw_ptr[v], v in [0, n]: the first of the n_entries distinct keys that is >= v << 32 (the sentinels lie at n << 32 | n, past
// every row; n_entries counts them out)
__global__ __launch_bounds__(MESH_BLOCK) void mesh_row_kernel(size_t base, const unsigned long long *__restrict__ unique, uint32_t n_entries,
                                                              size_t n, uint32_t *__restrict__ raw_ptr)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v > n) return;
    const unsigned long long want = (unsigned long long)v << 32;
    uint32_t lo = 0, hi = n_entries;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (unique[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    raw_ptr[v] = lo;
}

// the entries of row v that the header's N(v) keeps, counted (fill == nullptr) or written to fill in their order
__device__ __forceinline__ uint32_t mesh_row_neighbours(const uint32_t *__restrict__ raw_ptr, const unsigned long long *__restrict__ unique,
                                                        const uint32_t *__restrict__ times, size_t v, int boundary, uint32_t *__restrict__ fill)
{
    const uint32_t first = raw_ptr[v], last = raw_ptr[v + 1];
    bool on_boundary = false;
    for (uint32_t e = first; e < last; e++) on_boundary |= times[e] == 1;
    if (on_boundary && !boundary) return 0;
    uint32_t kept = 0;
    for (uint32_t e = first; e < last; e++) {
        if (on_boundary && times[e] != 1) continue;
        if (fill) fill[kept] = (uint32_t)unique[e];
        kept++;
    }
    return kept;
}

// degree[v] = |N(v)|, v in [0, n); degree[n] = 0 (the exclusive sum's last entry is the total)
__global__ __launch_bounds__(MESH_BLOCK) void mesh_degree_kernel(size_t base, const uint32_t *__restrict__ raw_ptr,
                                                                 const unsigned long long *__restrict__ unique, const uint32_t *__restrict__ times,
                                                                 size_t n, int boundary, uint32_t *__restrict__ degree)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v > n) return;
    degree[v] = v < n ? mesh_row_neighbours(raw_ptr, unique, times, v, boundary, nullptr) : 0u;
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_fill_kernel(size_t base, const uint32_t *__restrict__ raw_ptr,
                                                               const unsigned long long *__restrict__ unique, const uint32_t *__restrict__ times,
                                                               size_t n, int boundary, const uint32_t *__restrict__ ptr, uint32_t *__restrict__ col)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= n) return;
    mesh_row_neighbours(raw_ptr, unique, times, v, boundary, col + ptr[v]);
}

// the passes' working copy: STRIDE floats per vertex, 3 (the mesh's own layout, the default) or 4 (16-byte rows, the fourth float
// never read as a number: a neighbour is one 16-byte load instead of three 4-byte ones; measured slower)
template <int STRIDE> struct MeshPoint;
template <> struct MeshPoint<3> {
    static __device__ __forceinline__ void load(const float *__restrict__ p, size_t v, float x[3])
    {
        x[0] = p[3 * v]; x[1] = p[3 * v + 1]; x[2] = p[3 * v + 2];
    }
    static __device__ __forceinline__ void store(float *__restrict__ p, size_t v, const float x[3])
    {
        p[3 * v] = x[0]; p[3 * v + 1] = x[1]; p[3 * v + 2] = x[2];
    }
};
template <> struct MeshPoint<4> {
    static __device__ __forceinline__ void load(const float *__restrict__ p, size_t v, float x[3])
    {
        const float4 q = reinterpret_cast<const float4 *>(p)[v];
        x[0] = q.x; x[1] = q.y; x[2] = q.z;
    }
    static __device__ __forceinline__ void store(float *__restrict__ p, size_t v, const float x[3])
    {
        reinterpret_cast<float4 *>(p)[v] = make_float4(x[0], x[1], x[2], 0.0f);
    }
};

// 3 floats per vertex <-> 4 floats per vertex
__global__ __launch_bounds__(MESH_BLOCK) void mesh_pad_kernel(size_t base, const float *__restrict__ xyz, float *__restrict__ padded, size_t n)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= n) return;
    float x[3];
    MeshPoint<3>::load(xyz, v, x);
    MeshPoint<4>::store(padded, v, x);
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_unpad_kernel(size_t base, const float *__restrict__ padded, float *__restrict__ xyz, size_t n)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= n) return;
    float x[3];
    MeshPoint<4>::load(padded, v, x);
    MeshPoint<3>::store(xyz, v, x);
}

// One pass with factor f, the hot path: out[v] = (float)(x + f * (m - x)) per axis in f64, m the mean over N(v) of the previous
// pass's positions, summed in ascending index from +0; a vertex with empty N(v) is copied.  Every line is one rounded f64
// operation (-ffp-contract=off).
template <int STRIDE>
__global__ __launch_bounds__(MESH_BLOCK) void mesh_pass_kernel(size_t base, size_t n, const uint32_t *__restrict__ ptr,
                                                               const uint32_t *__restrict__ col, const float *__restrict__ in,
                                                               float *__restrict__ out, double f)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= n) return;
    const uint32_t first = ptr[v], last = ptr[v + 1];
    float x[3];
    MeshPoint<STRIDE>::load(in, v, x);
    if (first != last) {
        double s[3] = { 0.0, 0.0, 0.0 };
#pragma unroll 4                // four neighbours' loads in flight; the adds keep their order
        for (uint32_t e = first; e < last; e++) {
            float w[3];
            MeshPoint<STRIDE>::load(in, col[e], w);
#pragma unroll
            for (int k = 0; k < 3; k++) s[k] = s[k] + (double)w[k];
        }
        const double count = (double)(last - first);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double m = s[k] / count;
            const double d = m - (double)x[k];
            const double step = f * d;
            x[k] = (float)((double)x[k] + step);
        }
    }
    MeshPoint<STRIDE>::store(out, v, x);
}

// ---- clustering -----------------------------------------------------------------------------------------------------------------

struct MeshBounds {
    float lo[3], hi[3];
    unsigned long long bad;         // coordinates that are not finite
};

__device__ __forceinline__ void mesh_bounds_merge(MeshBounds &a, const MeshBounds &b)
{
#pragma unroll
    for (int k = 0; k < 3; k++) { a.lo[k] = fminf(a.lo[k], b.lo[k]); a.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
    a.bad += b.bad;
}

// the block's result from its threads' (min, max and a count: the order of the merges does not change the values)
__device__ __forceinline__ void mesh_bounds_block(MeshBounds &mine, MeshBounds *__restrict__ out)
{
    __shared__ MeshBounds part[MESH_BLOCK];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int half = MESH_BLOCK / 2; half > 0; half /= 2) {
        if ((int)threadIdx.x < half) mesh_bounds_merge(part[threadIdx.x], part[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

__device__ __forceinline__ MeshBounds mesh_bounds_empty()
{
    MeshBounds b;
#pragma unroll
    for (int k = 0; k < 3; k++) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
    b.bad = 0;
    return b;
}

// gridDim.x <= MESH_BOUNDS_BLOCKS blocks stride over the vertices; partial[blockIdx.x] is the block's result
__global__ __launch_bounds__(MESH_BLOCK) void mesh_bounds_kernel(const float *__restrict__ xyz, size_t n, MeshBounds *__restrict__ partial)
{
    MeshBounds mine = mesh_bounds_empty();
    for (size_t v = (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x; v < n; v += (size_t)gridDim.x * MESH_BLOCK) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float x = xyz[3 * v + k];
            if (isfinite(x)) { mine.lo[k] = fminf(mine.lo[k], x); mine.hi[k] = fmaxf(mine.hi[k], x); }
            else mine.bad++;
        }
    }
    mesh_bounds_block(mine, partial + blockIdx.x);
}

// one block: the n_partial partial results into result[0]
__global__ __launch_bounds__(MESH_BLOCK) void mesh_bounds_final_kernel(const MeshBounds *__restrict__ partial, int n_partial, MeshBounds *__restrict__ result)
{
    MeshBounds mine = mesh_bounds_empty();
    for (int i = threadIdx.x; i < n_partial; i += MESH_BLOCK) mesh_bounds_merge(mine, partial[i]);
    mesh_bounds_block(mine, result);
}

struct MeshCells {
    double lo[3], cell;
    unsigned long long count[3];    // cells per axis, each <= 2^21
};

// key = (c_z n_y + c_y) n_x + c_x, c = (int64)floor(((double)x - lo) / cell) per axis; order[v] = v
__global__ __launch_bounds__(MESH_BLOCK) void mesh_cell_keys_kernel(size_t base, const float *__restrict__ xyz, size_t n, const MeshCells g,
                                                                    unsigned long long *__restrict__ keys, uint32_t *__restrict__ order)
{
    const size_t v = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= n) return;
    unsigned long long c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double d = (double)xyz[3 * v + k] - g.lo[k];
        const double q = d / g.cell;
        c[k] = (unsigned long long)(long long)floor(q);
    }
    keys[v] = (c[2] * g.count[1] + c[1]) * g.count[0] + c[0];
    order[v] = (uint32_t)v;
}

// One thread per cluster k: its members are members[first[k] .. first[k + 1]) in ascending old index (the sort is stable).  Per
// axis S = the sum of the members' (double)x in that order from +0, position (float)(S / (double)count); cluster_of[member] = k.
// Sequential within a cluster, as the header's order of the sum is.
__global__ __launch_bounds__(MESH_BLOCK) void mesh_cluster_kernel(size_t base, const float *__restrict__ xyz, const uint32_t *__restrict__ members,
                                                                  const uint32_t *__restrict__ first, size_t n_clusters,
                                                                  float *__restrict__ out, uint32_t *__restrict__ cluster_of)
{
    const size_t k = base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (k >= n_clusters) return;
    const uint32_t begin = first[k], end = first[k + 1];
    double s[3] = { 0.0, 0.0, 0.0 };
    for (uint32_t i = begin; i < end; i++) {
        const size_t v = members[i];
#pragma unroll
        for (int a = 0; a < 3; a++) s[a] = s[a] + (double)xyz[3 * v + a];
        cluster_of[v] = (uint32_t)k;
    }
    const double count = (double)(end - begin);
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * k + a] = (float)(s[a] / count);
}

// a triangle's new indices; false when they are not all distinct (the triangle is dropped)
__device__ __forceinline__ bool mesh_triangle_image(const uint32_t *__restrict__ triangles, const uint32_t *__restrict__ cluster_of, size_t t,
                                                    size_t n_triangles, uint32_t abc[3])
{
    if (t >= n_triangles) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) abc[k] = cluster_of[triangles[3 * t + k]];
    return abc[0] != abc[1] && abc[1] != abc[2] && abc[2] != abc[0];
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_triangle_count_kernel(size_t base, const uint32_t *__restrict__ triangles,
                                                                         const uint32_t *__restrict__ cluster_of, size_t n_triangles,
                                                                         unsigned long long *__restrict__ block_count)
{
    using Reduce = hipcub::BlockReduce<uint32_t, MESH_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    uint32_t abc[3];
    const uint32_t keep = mesh_triangle_image(triangles, cluster_of, base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x, n_triangles, abc) ? 1u : 0u;
    const uint32_t sum = Reduce(tmp).Sum(keep);
    if (threadIdx.x == 0) block_count[base / MESH_BLOCK + blockIdx.x] = sum;
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_triangle_emit_kernel(size_t base, const uint32_t *__restrict__ triangles,
                                                                        const uint32_t *__restrict__ cluster_of, size_t n_triangles,
                                                                        const unsigned long long *__restrict__ block_offset,
                                                                        uint32_t *__restrict__ out)
{
    using Scan = hipcub::BlockScan<uint32_t, MESH_BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    uint32_t abc[3], first;
    const bool keep = mesh_triangle_image(triangles, cluster_of, base + (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x, n_triangles, abc);
    Scan(tmp).ExclusiveSum(keep ? 1u : 0u, first);
    if (!keep) return;
    uint32_t *o = out + 3 * ((size_t)block_offset[base / MESH_BLOCK + blockIdx.x] + first);
    o[0] = abc[0]; o[1] = abc[1]; o[2] = abc[2];
}
