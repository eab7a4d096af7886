// k_iso.hip.h -- the kernels of frog_isosurface_* (frog_chain.h): marching tetrahedra on the Kuhn decomposition of every grid
// cell.  Included by chain.hip inside its anonymous namespace, after NodeGrid (chain.hip includes <hipcub/hipcub.hpp> for it).
//
// Three passes over the nodes, x fastest, 256 consecutive nodes per block, and two exclusive sums over the blocks' totals
// between the first and the other two:
//   iso_classify_kernel   8 corner reads -> the cell's 8-bit configuration and the node's 7-bit edge mask, one byte each, and the
//                         block's vertex and triangle totals
//   iso_vertices_kernel   block scan of popcount(mask) + the block's offset -> vertex_offset[node], and the node's vertices
//   iso_triangles_kernel  block scan of the cell's triangle count + the block's offset -> the cell's triangles, each index
//                         vertex_offset[owner] + popcount(mask[owner] & ((1 << code) - 1))
// No hashing, no atomics: the output is a function of the input alone.
#pragma once

constexpr int ISO_BLOCK = 256;

// The 6 x 16 table of the rule in frog_chain.h, built from that rule at compile time.  tri[t][m] holds the triangles of
// tetrahedron t (the permutations of the axes in lexicographic order) with inside set m (bit q: tetrahedron vertex q), three
// bytes per triangle, each (owner corner) | (edge code) << 3 with corner = dx + 2 dy + 4 dz inside the cell.  corner[t][q] is
// the cube corner of tetrahedron vertex q.
struct IsoTable {
    uint8_t tri[6][16][6];
    uint8_t corner[6][4];
};

constexpr IsoTable iso_make_table()
{
    IsoTable T{};
    const int perms[6][3] = { { 0, 1, 2 }, { 0, 2, 1 }, { 1, 0, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 2, 1, 0 } };
    for (int t = 0; t < 6; t++) {
        int V[4][3] = {};
        V[1][perms[t][0]] = 1;
        for (int k = 0; k < 3; k++) { V[2][k] = V[1][k]; V[3][k] = 1; }
        V[2][perms[t][1]] += 1;
        for (int q = 0; q < 4; q++) T.corner[t][q] = (uint8_t)(V[q][0] + 2 * V[q][1] + 4 * V[q][2]);
        for (int m = 1; m < 15; m++) {
            int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
            for (int q = 0; q < 4; q++) {
                if (m >> q & 1) in[n_in++] = q;
                else out[n_out++] = q;
            }
            // the triangles' vertices as pairs of tetrahedron vertex numbers
            int pair[2][3][2] = {}, n_tri = 1;
            if (n_in == 1) {
                for (int v = 0; v < 3; v++) { pair[0][v][0] = in[0]; pair[0][v][1] = out[v]; }
            } else if (n_in == 3) {
                for (int v = 0; v < 3; v++) { pair[0][v][0] = in[v]; pair[0][v][1] = out[0]; }
            } else {
                const int a = in[0], b = in[1], c = out[0], d = out[1];
                const int quad[2][3][2] = { { { a, c }, { a, d }, { b, d } }, { { a, c }, { b, d }, { b, c } } };
                n_tri = 2;
                for (int r = 0; r < 2; r++)
                    for (int v = 0; v < 3; v++) { pair[r][v][0] = quad[r][v][0]; pair[r][v][1] = quad[r][v][1]; }
            }
            // n_in * n_out * (mean of the outside corners - mean of the inside corners): the same sign, in integers
            int d[3] = {};
            for (int k = 0; k < 3; k++) {
                int s_in = 0, s_out = 0;
                for (int q = 0; q < n_in; q++) s_in += V[in[q]][k];
                for (int q = 0; q < n_out; q++) s_out += V[out[q]][k];
                d[k] = n_in * s_out - n_out * s_in;
            }
            for (int r = 0; r < n_tri; r++) {
                int mid[3][3] = {};         // twice the edge midpoints
                for (int v = 0; v < 3; v++)
                    for (int k = 0; k < 3; k++) mid[v][k] = V[pair[r][v][0]][k] + V[pair[r][v][1]][k];
                int e1[3] = {}, e2[3] = {};
                for (int k = 0; k < 3; k++) { e1[k] = mid[1][k] - mid[0][k]; e2[k] = mid[2][k] - mid[0][k]; }
                const int nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
                const bool flip = nx * d[0] + ny * d[1] + nz * d[2] <= 0;
                for (int v = 0; v < 3; v++) {
                    const int w = flip ? (3 - v) % 3 : v;       // 0, 2, 1
                    const int p = pair[r][w][0], q = pair[r][w][1];
                    const int lo = p < q ? p : q, hi = p < q ? q : p;   // the tetrahedron's vertices ascend along the cube's diagonal
                    const int code = (V[hi][0] - V[lo][0]) + 2 * (V[hi][1] - V[lo][1]) + 4 * (V[hi][2] - V[lo][2]) - 1;
                    T.tri[t][m][3 * r + v] = (uint8_t)(T.corner[t][lo] | code << 3);
                }
            }
        }
    }
    return T;
}

__constant__ IsoTable ISO_TABLE = iso_make_table();

// triangles of a tetrahedron with inside set m: 0, 1 (one or three inside) or 2 (two inside)
__device__ __forceinline__ uint32_t iso_tet_triangles(uint32_t m)
{
    const uint32_t n = __popc(m);
    return n == 2 ? 2u : (n == 1 || n == 3 ? 1u : 0u);
}

// the inside set of tetrahedron t in a cell of configuration config (t is a constant wherever this is called: the corner
// numbers fold)
__device__ __forceinline__ uint32_t iso_tet_case(uint32_t config, int t)
{
    constexpr IsoTable T = iso_make_table();
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) m |= (config >> T.corner[t][q] & 1u) << q;
    return m;
}

struct IsoParams {
    NodeGrid g;
    int mode;
    double level;
    long long value;
};

template <class S>
__device__ __forceinline__ bool iso_inside(const IsoParams &p, S v)
{
    if (p.mode == FROG_ISO_LABEL) {
        if constexpr (std::is_integral<S>::value) return (long long)v == p.value;
        else return false;
    }
    return (double)v >= p.level;        // false for a NaN
}

// The node's index per axis; false past the grid.
__device__ __forceinline__ bool iso_node(const NodeGrid &g, size_t idx, size_t total, uint32_t ijk[3])
{
    if (idx >= total) return false;
    const uint32_t nx = g.dims[0], ny = g.dims[1];
    ijk[0] = (uint32_t)(idx % nx); ijk[1] = (uint32_t)((idx / nx) % ny); ijk[2] = (uint32_t)(idx / ((size_t)nx * ny));
    return true;
}

// Pass 1.  A corner past the grid takes the node's own bit, so its edge does not cross; a node on the grid's upper border
// owns no cell.  config is stored only for nodes that own a cell (0 otherwise: no triangle).
template <class S>
__global__ __launch_bounds__(ISO_BLOCK) void iso_classify_kernel(size_t base, const S *__restrict__ vol, size_t total, const IsoParams p,
                                                                 uint8_t *__restrict__ mask, uint8_t *__restrict__ config,
                                                                 unsigned long long *__restrict__ block_vertices,
                                                                 unsigned long long *__restrict__ block_triangles)
{
    using Reduce = hipcub::BlockReduce<uint32_t, ISO_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp_v, tmp_t;
    const size_t idx = base + (size_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
    uint32_t ijk[3], n_v = 0, n_t = 0;
    if (iso_node(p.g, idx, total, ijk)) {
        const uint32_t nx = p.g.dims[0], ny = p.g.dims[1], nz = p.g.dims[2];
        const bool ex = ijk[0] + 1 < nx, ey = ijk[1] + 1 < ny, ez = ijk[2] + 1 < nz;
        const uint32_t own = iso_inside(p, vol[idx]) ? 1u : 0u;
        uint32_t c = own;
#pragma unroll
        for (int k = 1; k < 8; k++) {
            const bool exists = (!(k & 1) || ex) && (!(k & 2) || ey) && (!(k & 4) || ez);
            uint32_t bit = own;
            if (exists) bit = iso_inside(p, vol[idx + (k & 1) + (size_t)nx * ((k >> 1 & 1) + (size_t)ny * (k >> 2 & 1))]) ? 1u : 0u;
            c |= bit << k;
        }
        const uint32_t m = ((c >> 1) ^ (own ? 0x7fu : 0u)) & 0x7fu;
        if (!(ex && ey && ez)) c = 0;
        n_v = __popc(m);
#pragma unroll
        for (int t = 0; t < 6; t++) n_t += iso_tet_triangles(iso_tet_case(c, t));
        mask[idx] = (uint8_t)m;
        config[idx] = (uint8_t)c;
    }
    const uint32_t sum_v = Reduce(tmp_v).Sum(n_v), sum_t = Reduce(tmp_t).Sum(n_t);
    if (threadIdx.x == 0) {
        const size_t block = base / ISO_BLOCK + blockIdx.x;
        block_vertices[block] = sum_v;
        block_triangles[block] = sum_t;
    }
}

// Pass 2.  The vertex on the edge from node a (the owner) to b = a + (dx, dy, dz): t in f64, p = pa + t * (pb - pa) per axis in
// f64, one cast.
template <class S>
__global__ __launch_bounds__(ISO_BLOCK) void iso_vertices_kernel(size_t base, const S *__restrict__ vol, size_t total, const IsoParams p,
                                                                 const uint8_t *__restrict__ mask,
                                                                 const unsigned long long *__restrict__ block_offset,
                                                                 uint32_t *__restrict__ vertex_offset, float *__restrict__ xyz)
{
    using Scan = hipcub::BlockScan<uint32_t, ISO_BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    const size_t idx = base + (size_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
    uint32_t ijk[3];
    const bool live = iso_node(p.g, idx, total, ijk);
    const uint32_t m = live ? mask[idx] : 0u;
    uint32_t first;
    Scan(tmp).ExclusiveSum((uint32_t)__popc(m), first);
    if (!live) return;
    first += (uint32_t)block_offset[base / ISO_BLOCK + blockIdx.x];
    vertex_offset[idx] = first;
    if (!m) return;
    const uint32_t nx = p.g.dims[0], ny = p.g.dims[1];
    const double va = (double)vol[idx];
    double pa[3];
#pragma unroll
    for (int k = 0; k < 3; k++) pa[k] = p.g.origin[k] + ijk[k] * p.g.spacing[k];
    for (uint32_t code = 0; code < 7; code++) {
        if (!(m >> code & 1u)) continue;
        const uint32_t d[3] = { (code + 1) & 1u, (code + 1) >> 1 & 1u, (code + 1) >> 2 & 1u };
        double t = 0.5;
        if (p.mode == FROG_ISO_LEVEL) {
            const double vb = (double)vol[idx + d[0] + (size_t)nx * (d[1] + (size_t)ny * d[2])];
            if (isfinite(va) && isfinite(vb)) t = (p.level - va) / (vb - va);
        }
        float *out = xyz + 3 * (size_t)first;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double pb = p.g.origin[k] + (ijk[k] + d[k]) * p.g.spacing[k];
            out[k] = (float)(pa[k] + t * (pb - pa[k]));
        }
        first++;
    }
}

// Pass 3.
__global__ __launch_bounds__(ISO_BLOCK) void iso_triangles_kernel(size_t base, size_t total, const NodeGrid g, const uint8_t *__restrict__ mask,
                                                                  const uint8_t *__restrict__ config,
                                                                  const unsigned long long *__restrict__ block_offset,
                                                                  const uint32_t *__restrict__ vertex_offset, uint32_t *__restrict__ triangles)
{
    using Scan = hipcub::BlockScan<uint32_t, ISO_BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    const size_t idx = base + (size_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
    const uint32_t c = idx < total ? config[idx] : 0u;
    uint32_t cases[6], n_t = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) { cases[t] = iso_tet_case(c, t); n_t += iso_tet_triangles(cases[t]); }
    uint32_t first;
    Scan(tmp).ExclusiveSum(n_t, first);
    if (!n_t) return;
    uint32_t *out = triangles + 3 * ((size_t)block_offset[base / ISO_BLOCK + blockIdx.x] + first);
    const size_t nx = g.dims[0], ny = g.dims[1];
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const uint32_t n = 3 * iso_tet_triangles(cases[t]);
        for (uint32_t v = 0; v < n; v++) {
            const uint32_t e = ISO_TABLE.tri[t][cases[t]][v], corner = e & 7u, code = e >> 3;
            const size_t owner = idx + (corner & 1u) + nx * ((corner >> 1 & 1u) + ny * (corner >> 2 & 1u));
            *out++ = vertex_offset[owner] + __popc(mask[owner] & ((1u << code) - 1u));
        }
    }
}

// frog_chain_apply_f32: frog_chain_apply on the widened point, cast once; in and out may be the same array
__global__ __launch_bounds__(256) void chain_apply_f32_kernel(size_t base, const DevLink *links, int n_links, const float *in, float *out, size_t n)
{
    const size_t i = base + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[3] = { (double)in[3 * i], (double)in[3 * i + 1], (double)in[3 * i + 2] }, A[3][3];
    chain_point<false>(links, n_links, p, A);
    out[3 * i] = (float)p[0]; out[3 * i + 1] = (float)p[1]; out[3 * i + 2] = (float)p[2];
}
