// k_joint.hip.h -- joint label fusion (frog_jlabels, include/frog_chain.h, which states the arithmetic line by line): the
// kernel of finish.  Included by chain.hip inside its anonymous namespace, after the label map and label_load it reuses.
//
// Mapping.  A block is one wavefront and owns a tile: a run of JL_RUN voxels along x.  The wavefront is cut into groups of G
// lanes, and a group works on one voxel at a time, so 64 / G voxels are in flight.  N(N+1)/2 accumulators do not fit one
// thread, so the lanes of a group share them: pair p = lane + G k (k < PPL) of the lower triangle, row by row, belongs to
// that lane for the whole patch walk, in PPL registers whose every index is a compile-time constant.  The header fixes the
// order of the adds inside an entry only, so this ownership gives the stated bits.
//
// Per voxel: (1) lane x <= N walks the patch of plane x (0: the target, i + 1: atlas i) for n, s, ss and leaves mean and inv
// in LDS; a ballot of the centres' validity is the active set.  (2) Per patch row (dz, dy) the group writes the (2R+1) N
// differences d_i(u) to LDS, then every lane adds the products of its pairs, tap by tap.  (3) The powers and alpha go to the
// packed lower triangle K in LDS.  (4) LDL^T in place, lane i owning row i: at column j every lane forms D_j from the same
// broadcast reads as its own x -- the same rounded sequence in every lane -- and row i's L_ij replaces K_ij.  The forward
// sweep is by columns (lane i subtracts L_ik z_k for k ascending as z_k becomes final).  The backward sweep needs w_k for
// every k > i before row i's sum, whose subtractions run over k ascending: when w_k is final the lanes i < k replace L_ki by
// the product L_ki w_k, and lane i later subtracts the stored products in ascending k.  K never leaves the chip.
//
// The active set differs between the voxels of a wavefront, the trip counts may not: all N rows stay, with L_ij = +0.0 where
// atlas i or j is not active and D_j = 1, z_j = y_j = w_j = +0.0 where j is not.  What such a row contributes to an active
// one is (+0.0 * +0.0) * 1 = +0.0, and x - (+0.0) is x for every x: the active rows carry the bits of the restricted system.
// A tap outside the grid or not valid is a NaN and adds nothing; a d of +0.0 adds +0.0 to an M that is never -0.0.
//
// Planes.  Where (N + 1) planes of the run and its halo, (JL_RUN + 2R) x (2R+1)^2 floats each, fit JL_LDS_BUDGET beside the
// groups' scratch, the block stages them in LDS and both passes over the patch read them there; where they do not (from
// N = 23 at R = 2, N = 10 at R = 3) a tap is a bounds-checked read through the cache.  The Gram pass, which dominates, reads
// only the row's differences in either case.  Every barrier is a __syncthreads() of a one-wavefront block.
#pragma once

constexpr int JL_RUN = 8;                           // voxels of a tile, along x
constexpr int JL_MAX_N = 32;
constexpr size_t JL_LDS_BUDGET = 32 * 1024;         // bytes of LDS a block may take and still stage: five blocks per CU

struct JointArgs {
    const float *target;                            // the target's plane, NaN where not valid
    const float *atlases;                           // n planes of `total`
    const void *const *labels;                      // n label maps on the grid
    const int *ltypes;                              // their voxel types
    float *weights;                                 // n planes, or null
    float *const *planes;                           // dense label index -> score plane
    uint32_t n_planes;
    LabelMap map;
    size_t total, tiles;
    uint32_t nx, ny, nz, runs;                      // the grid; tiles along x
    int n, radius, beta, staged;
    double alpha;
};

// doubles of LDS of one group: K, a row's differences, D, mean and inv of the N + 1 planes, z / w, and (label, weight)
__host__ __device__ inline size_t joint_group_doubles(int n, int radius)
{
    return (size_t)n * (n + 1) / 2 + (size_t)(2 * radius + 1) * n + n + 2 * (size_t)(n + 1) + n + n;
}

__host__ __device__ inline size_t joint_staged_floats(int n, int radius)
{
    const size_t w = 2 * radius + 1;
    return (size_t)(n + 1) * (JL_RUN + 2 * radius) * w * w;
}

__device__ __forceinline__ int joint_tri(int i, int j) { return i * (i + 1) / 2 + j; }

template <int G, int PPL>
__global__ __launch_bounds__(64) void jlabels_solve_kernel(size_t base, const JointArgs a)
{
    extern __shared__ double jl_mem[];
    constexpr int GROUPS = 64 / G;
    const size_t tile = base / 256 + blockIdx.x;            // one block per tile: the same for every thread of the block
    if (tile >= a.tiles) return;
    const int N = a.n, R = a.radius, W = 2 * R + 1, P = N * (N + 1) / 2;
    const int x0 = (int)(tile % a.runs) * JL_RUN, y0 = (int)((tile / a.runs) % a.ny), z0 = (int)(tile / ((size_t)a.runs * a.ny));
    const int lane = threadIdx.x % G, group = threadIdx.x / G;
    double *const Kt = jl_mem + (size_t)group * joint_group_doubles(N, R);
    double *const db = Kt + P;
    double *const Dv = db + W * N;
    double *const mean = Dv + N;
    double *const inv = mean + N + 1;
    double *const wv = inv + N + 1;
    uint32_t *const labs = (uint32_t *)(wv + N);
    float *const wfs = (float *)(labs + N);
    const float *const s_planes = (const float *)(jl_mem + (size_t)GROUPS * joint_group_doubles(N, R));
    const int HX = JL_RUN + 2 * R, PE = HX * W * W;
    const float nan = __builtin_nanf("");

    if (a.staged) {
        float *const stage = (float *)(jl_mem + (size_t)GROUPS * joint_group_doubles(N, R));
        for (int e = threadIdx.x; e < (N + 1) * PE; e += 64) {
            const int p = e / PE, r = e % PE;
            const int x = x0 - R + r % HX, y = y0 - R + (r / HX) % W, z = z0 - R + r / (HX * W);
            float v = nan;
            if (x >= 0 && y >= 0 && z >= 0 && x < (int)a.nx && y < (int)a.ny && z < (int)a.nz) {
                const size_t idx = (size_t)x + (size_t)a.nx * ((size_t)y + (size_t)a.ny * (size_t)z);
                v = p ? a.atlases[(size_t)(p - 1) * a.total + idx] : a.target[idx];
            }
            stage[e] = v;
        }
    }
    __syncthreads();

    // plane p at tap (dx, dy, dz) of the patch around voxel lx of the run; NaN where there is no valid voxel
    auto tap = [&](int p, int lx, int dx, int dy, int dz) -> float {
        if (a.staged) return s_planes[p * PE + (dz * W + dy) * HX + lx + dx];
        const int x = x0 + lx + dx - R, y = y0 + dy - R, z = z0 + dz - R;
        if (x < 0 || y < 0 || z < 0 || x >= (int)a.nx || y >= (int)a.ny || z >= (int)a.nz) return nan;
        const size_t idx = (size_t)x + (size_t)a.nx * ((size_t)y + (size_t)a.ny * (size_t)z);
        return p ? a.atlases[(size_t)(p - 1) * a.total + idx] : a.target[idx];
    };

    // the pairs of this lane: p = lane + G k, row by row of the lower triangle
    int pi[PPL], pj[PPL];
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        const int p = lane + G * k;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= p) i++;
        pi[k] = p < P ? i : 0;
        pj[k] = p < P ? p - i * (i + 1) / 2 : 0;
    }

    for (int it = 0; it < JL_RUN / GROUPS; it++) {
        const int lx = it * GROUPS + group;
        const bool live = x0 + lx < (int)a.nx;
        const size_t idx = (size_t)(x0 + lx) + (size_t)a.nx * ((size_t)y0 + (size_t)a.ny * (size_t)z0);

        // (1) patch statistics of plane `lane`, and the active set
        bool centre = false;
        if (lane <= N) {
            double n = 0.0, s = 0.0, ss = 0.0;
            for (int dz = 0; dz < W; dz++)
                for (int dy = 0; dy < W; dy++)
                    for (int dx = 0; dx < W; dx++) {
                        const float f = tap(lane, lx, dx, dy, dz);
                        if (f == f) {
                            const double X = (double)f, XX = X * X;
                            n = n + 1.0; s = s + X; ss = ss + XX;
                        }
                    }
            const double nss = n * ss, s2 = s * s, nn = n * n, num = nss - s2;
            const double var = num / nn;
            mean[lane] = s / n;
            double v = 0.0;
            if (n >= 2.0 && var > 0.0) {
                const double sd = sqrt(var);
                v = 1.0 / sd;
            }
            inv[lane] = v;
            const float c = tap(lane, lx, R, R, R);
            centre = live && c == c;
        }
        const unsigned long long ballot = __ballot(centre);
        // bit 0 of the group's share: the target; bit i + 1: atlas i
        const bool valid_t = (ballot >> (group * G)) & 1ull;
        auto active = [&](int i) -> bool { return valid_t && ((ballot >> (group * G + i + 1)) & 1ull); };
        const bool act = lane < N && active(lane);
        __syncthreads();

        // (2) the Gram matrix, one patch row at a time
        double acc[PPL];
#pragma unroll
        for (int k = 0; k < PPL; k++) acc[k] = 0.0;
        const double mean_t = mean[0], inv_t = inv[0];
        for (int dz = 0; dz < W; dz++) {
            for (int dy = 0; dy < W; dy++) {
                for (int e = lane; e < W * N; e += G) {
                    const int dx = e / N, i = e % N;
                    const float t = tap(0, lx, dx, dy, dz), f = tap(i + 1, lx, dx, dy, dz);
                    double d = 0.0;
                    if (t == t && f == f) {
                        const double ac = (double)f - mean[i + 1], ah = ac * inv[i + 1];
                        const double tc = (double)t - mean_t, th = tc * inv_t;
                        d = fabs(ah - th);
                    }
                    db[e] = d;
                }
                __syncthreads();
                for (int dx = 0; dx < W; dx++) {
                    const double *row = db + dx * N;
#pragma unroll
                    for (int k = 0; k < PPL; k++) {
                        const double p = row[pi[k]] * row[pj[k]];
                        acc[k] = acc[k] + p;
                    }
                }
                __syncthreads();
            }
        }

        // (3) K: the elementwise power, alpha on the diagonal
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const int p = lane + G * k;
            if (p < P) {
                double v = acc[k];
                for (int b = 1; b < a.beta; b++) v = v * acc[k];
                if (pi[k] == pj[k]) v = v + a.alpha;
                Kt[p] = v;
            }
        }
        __syncthreads();

        // (4) LDL^T in place: lane i owns row i
        const bool row = lane < N;
        for (int j = 0; j < N; j++) {
            const bool act_j = active(j), mine = row && lane > j;
            const double *Lj = Kt + joint_tri(j, 0), *Li = Kt + joint_tri(mine ? lane : j, 0);
            double dj = Lj[j], x = Li[j];
            for (int k = 0; k < j; k++) {
                const double ljk = Lj[k], lik = Li[k], dk = Dv[k];
                const double qj = ljk * ljk, mj = qj * dk;
                dj = dj - mj;
                const double qi = lik * ljk, mi = qi * dk;
                x = x - mi;
            }
            if (!act_j) dj = 1.0;
            if (lane == j) Dv[j] = dj;
            if (mine) Kt[joint_tri(lane, j)] = act && act_j ? x / dj : 0.0;
            __syncthreads();
        }
        double zi = 1.0;
        for (int k = 0; k < N; k++) {
            if (lane == k) wv[k] = act ? zi : 0.0;
            __syncthreads();
            if (row && lane > k) {
                const double m = Kt[joint_tri(lane, k)] * wv[k];
                zi = zi - m;
            }
        }
        const double yi = act ? zi / Dv[lane] : 0.0;
        __syncthreads();
        double wi = 0.0;
        for (int i = N - 1; i >= 0; i--) {
            if (lane == i) {
                wi = yi;
                for (int k = i + 1; k < N; k++) wi = wi - Kt[joint_tri(k, i)];
                if (!act) wi = 0.0;
                wv[i] = wi;
            }
            __syncthreads();
            if (lane < i) {
                const double m = Kt[joint_tri(i, lane)] * wv[i];
                Kt[joint_tri(i, lane)] = m;
            }
            __syncthreads();
        }
        double S = 0.0;
        for (int i = 0; i < N; i++) S = S + wv[i];
        float wf = 0.0f;
        if (act) {
            const double wn = wi / S;
            wf = (float)wn;
        }

        // the weight plane and the votes, in call order per label: the first atlas of a label writes the label's sum
        if (row) {
            labs[lane] = act ? label_find(a.map, label_load(a.labels[lane], a.ltypes[lane], idx)) : 0xffffffffu;
            wfs[lane] = wf;
            if (a.weights && live) a.weights[(size_t)lane * a.total + idx] = wf;
        }
        __syncthreads();
        if (act) {
            const uint32_t l = labs[lane];
            bool first = true;
            float score = 0.0f;
            for (int k = 0; k < N; k++) {
                if (labs[k] != l) continue;
                if (k < lane) first = false;
                score = score + wfs[k];
            }
            if (first && l < a.n_planes) a.planes[l][idx] = score;
        }
        __syncthreads();
    }
}
