// k_comm.hip.h -- the device side of the sharded contexts' coordinate exchange (include/frog_hip.h frog_comm_unpack_slab,
// frog_comm_unpack_slab_step, frog_transform_points_slab): slab slots -> the coordinate table, the slots' trailers.
#pragma once

#include "k_grid.hip.h"

namespace frog {

// the trailer of a context that launches no transform that would write it (no point owned, fresh lattice, reference-order mode)
__global__ void slab_trailer_kernel(const double *energy, double *trailer) { write_slab_trailer(energy, trailer); }

// rows [row_begin[r], row_begin[r + 1]) of every rank r != self: slab slot r -> the coordinate table
constexpr int UNPACK_MAX_RANKS = 64;
struct UnpackArgs {
    uint64_t row_begin[UNPACK_MAX_RANKS + 1];
    uint64_t slot_bytes;            // distance between two ranks' slots
    uint32_t world, self;           // self == world: the own rows are copied too (frog_comm_unpack_slab_step)
    // frog_comm_unpack_slab_step: the slots' trailers (N_SCALARS doubles at slot + trailer_off) are added up over the ranks for the
    // scalars in sum_mask and the step's four scalars handed to the host (k_grid.hip.h store_step_scalars)
    uint64_t trailer_off;
    uint32_t sum_mask;
    double *energy, *host_scalars;
    double seq;
};
// `snap` (null: no list to check): the block also leaves the largest distance of the rows it copies from the culling list's
// snapshot in disp_part[blockIdx.y * gridDim.x + blockIdx.x] (k_cull.hip.h: what cull_disp_kernel computes in a pass of its own)
__global__ __launch_bounds__(256) void unpack_slab_kernel(const P3 *slab, P3 *pos2, const UnpackArgs a, const P3 *snap, uint32_t *disp_part)
{
    __shared__ uint32_t sh[4];
    const uint32_t r = blockIdx.y;
    if (a.sum_mask && blockIdx.x == 0 && r == 0 && threadIdx.x == 0) {
        // the ranks' trailers in rank order: integers (oversize counts, flags) add exactly; the energy sums of a linear step
        // in the same order on every rank, so every rank prints the same E
        for (int k = 0; k < N_SCALARS; k++) {
            if (!(a.sum_mask >> k & 1u)) continue;
            double sum = 0.0;
            for (uint32_t q = 0; q < a.world; q++)
                sum += reinterpret_cast<const double *>(reinterpret_cast<const unsigned char *>(slab) + q * a.slot_bytes + a.trailer_off)[k];
            a.energy[k] = sum;
        }
        __threadfence();
        if (a.host_scalars) store_step_scalars(a.host_scalars, a.energy, a.seq);    // null: the host gets them by copy + event
    }
    uint32_t m = 0;
    if (r != a.self) {
        const uint64_t n = a.row_begin[r + 1] - a.row_begin[r];
        const P3 *slot = reinterpret_cast<const P3 *>(reinterpret_cast<const unsigned char *>(slab) + r * a.slot_bytes);
        for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256u) {
            const P3 v = slot[k];
            pos2[a.row_begin[r] + k] = v;
            if (snap) {
                const P3 q = snap[a.row_begin[r] + k];
                const float dx = v.x - q.x, dy = v.y - q.y, dz = v.z - q.z;
                m = max(m, __float_as_uint(__builtin_sqrtf(dx * dx + dy * dy + dz * dz)) & 0x7FFFFFFFu);
            }
        }
    }
    if (!snap) return;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) disp_part[blockIdx.y * gridDim.x + blockIdx.x] = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

} // namespace frog
