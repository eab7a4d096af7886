// rank_steps.h -- one rank's steps of a registration over the C ABI of libfrog_hip.so and, when the images are sharded, the
// collectives of libfrog_comm.so: the bodies of the loops of ImageGroup::run (registration/imageGroup.cxx:54-66, :78-128) in
// their three flavours.  The loops themselves are in rank_schedule.cpp (frog_run_schedule, timed) and image_group.cpp
// (bin/frog, printing and recording); the places where the reference's loops read another image's state are collectives
// here.  No solver arithmetic, no allocation inside a step.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/frog_hip.h"
#include "comm_api.h"

struct RankSteps {
    frog_ctx *c = nullptr;
    frog_comm *cm = nullptr;
    CommApi *api = nullptr;
    const float *proxy_em = nullptr;    // no communicator, a shard: the other ranks' rows of the mixture table (frog_schedule_plan)
    bool whole = false;             // the context owns every image and there is no communicator: the plain entry points
    // Two collectives per deformable iteration, one per linear iteration (include/frog_hip.h frog_comm_mode): the energy sums ride
    // on the all-reduce of the proposal sums, the oversize count on the coordinate gather, whose transform is queued speculatively.
    // FROG_THREE_COLLECTIVES=1 keeps the flow of rounds 2-4 (three / two), for comparison.
    bool two = false;
    bool gathered = false;          // the step just finished has already transformed and gathered: the transformPoints() that follows it is done
    // ... and the NEXT step's phase A is queued before this step's decision has reached the host (frog_step_speculate): the GPU
    // does not wait for the host's read + launch latency once per iteration.  FROG_NO_SPECULATION=1 switches it off.
    bool speculate = false;
    bool phaseAQueued = false;      // the coming deformableStep finds its phase A already in the queue
    uint32_t ib = 0, ie = 0, nI = 0;
    // Sticky: after the first call that fails every step returns at once, so the loops need no branch per call.
    int rc = 0;
    const char *failed = nullptr;   // the name of that call

    bool ok(int r, const char *call) { if (r && !rc) { rc = r; failed = call; } return rc == 0; }

    // `comm` null: one context alone.  With a communicator, libfrog_comm.so is loaded already (CommApi::load).  n_fixed: the
    // context was created with that many fixed images (-fi), which it keeps in a helper of its own and does not count as owned.
    int init(frog_ctx *ctx, frog_comm *comm, const float *proxy, uint32_t n_fixed = 0)
    {
        c = ctx; cm = comm; proxy_em = proxy;
        api = comm ? &host_comm_api() : nullptr;
        nI = frog_num_images(ctx);
        size_t b = 0, e = 0;
        if (!ok(frog_comm_buffer(ctx, FROG_BUF_EM, nullptr, nullptr, &b, &e), "frog_comm_buffer")) return rc;
        ib = (uint32_t)b; ie = (uint32_t)e;
        whole = !comm && ib == n_fixed && ie == nI;
        two = comm && !getenv("FROG_THREE_COLLECTIVES");
        speculate = two && !getenv("FROG_NO_SPECULATION");
        if (comm) ok(frog_comm_mode(ctx, two ? 1 : 0), "frog_comm_mode");
        return rc;
    }

    void transformPoints(int apply)
    {
        if (rc) return;
        if (whole) { ok(frog_transform_points(c, apply), "frog_transform_points"); return; }
        if (two) {
            const bool done = gathered && !apply;
            gathered = false;
            if (!done) ok(api->gather_points(cm, apply, 0, 0u), "frog_comm_gather_points");
            return;
        }
        if (!ok(frog_transform_points_local(c, apply), "frog_transform_points_local")) return;
        if (cm) ok(api->all_gather_xyz2(cm), "frog_comm_all_gather_xyz2");
    }
    void updateStats()
    {
        if (rc) return;
        if (whole) { ok(frog_update_stats(c), "frog_update_stats"); return; }
        if (!ok(frog_update_stats_local(c), "frog_update_stats_local")) return;
        if (cm) { if (!ok(api->all_reduce(cm, FROG_BUF_EM), "frog_comm_all_reduce")) return; }
        else if (proxy_em) {
            if (!ok(frog_set_em_rows(c, proxy_em, 0, ib), "frog_set_em_rows") || !ok(frog_set_em_rows(c, proxy_em, ie, nI), "frog_set_em_rows")) return;
        }
        ok(frog_stats_publish(c), "frog_stats_publish");
    }
    double linearStep()
    {
        double E = 0;
        if (rc) return E;
        if (whole) { ok(frog_linear_step(c, &E), "frog_linear_step"); return E; }
        if (!ok(frog_linear_step_local(c), "frog_linear_step_local")) return E;
        if (two) {
            // the step's two sums and its list flag travel in the trailers of the coordinate gather (imageGroup.cxx:1147 needs
            // them for the printed E only; the matrices are image-local): ONE collective per linear iteration
            if (!ok(api->gather_points(cm, 0, 0, 0xBu), "frog_comm_gather_points")) return E;
            ok(frog_step_finish(c, &E), "frog_step_finish");
            gathered = true;
            return E;
        }
        if (cm && !ok(api->all_reduce(cm, FROG_BUF_ENERGY), "frog_comm_all_reduce")) return E;
        ok(frog_energy_read(c, &E, nullptr), "frog_energy_read");
        return E;
    }
    void setup(int level, frog_grid_info &info)
    {
        if (rc) return;
        if (whole) { ok(frog_deformable_setup(c, level, &info), "frog_deformable_setup"); return; }
        double mn[3], mx[3];
        if (!ok(frog_bounds_local(c, mn, mx), "frog_bounds_local")) return;
        if (cm && !ok(api->all_reduce_bounds(cm, mn, mx), "frog_comm_all_reduce_bounds")) return;
        ok(frog_deformable_setup_bounds(c, level, mn, mx, &info), "frog_deformable_setup_bounds");
    }
    // next_plain: the iteration after this one, if this one is accepted, is an ordinary one (same level, no statistics refresh first)
    double deformableStep(float alpha, bool next_plain)
    {
        double E = 0;
        if (rc) return E;
        if (whole) { ok(frog_deformable_step(c, alpha, &E), "frog_deformable_step"); return E; }
        const bool queued = phaseAQueued;
        phaseAQueued = false;
        if (!queued && !ok(frog_deformable_phase_a(c, alpha), "frog_deformable_phase_a")) return E;
        if (cm && !ok(api->all_reduce(cm, FROG_BUF_GRIDSUM), "frog_comm_all_reduce")) return E;     // the shared common-space grid, :400-432 (+ the energy sums when `two`)
        if (!ok(frog_deformable_phase_b(c), "frog_deformable_phase_b")) return E;
        if (two) {
            // the transform that follows the step, queued before the group's oversize count exists (each rank goes by its own),
            // the counts in the gather's trailers; decision and commit once they are added up.  A rejected step has left
            // speculative coordinates in the replicas: the loop's reject path re-bases and gathers before anything reads them.
            if (!ok(api->gather_points(cm, 0, 1, 0x4u), "frog_comm_gather_points")) return E;
            if (speculate && next_plain) {
                if (!ok(frog_step_speculate(c), "frog_step_speculate") || !ok(frog_deformable_phase_a(c, alpha), "frog_deformable_phase_a")) return E;
                phaseAQueued = true;
            }
            ok(frog_step_finish(c, &E), "frog_step_finish");
            gathered = (float)E >= 0;
            if (!gathered) phaseAQueued = false;        // rejected: frog_step_finish has rolled the speculation back
            return E;
        }
        if (cm && !ok(api->all_reduce(cm, FROG_BUF_ENERGY), "frog_comm_all_reduce")) return E;      // energy sums + oversize count
        ok(frog_deformable_phase_c(c, &E), "frog_deformable_phase_c");
        return E;
    }
    void barrier() { if (cm && !rc) ok(api->barrier(cm), "frog_comm_barrier"); }        // of the ranks; nothing without a communicator
    // Every rank holds a replica of all transformed coordinates (the gather's product) and of the mixture table: FNV-1a over
    // their bit patterns, the same on every rank whatever carried the collectives.
    uint64_t replicaHash()
    {
        std::vector<float> v(3 * frog_num_points(c) + 3 * (size_t)nI);
        float *em = v.data() + 3 * frog_num_points(c);
        ok(frog_get_points(c, nullptr, v.data()), "frog_get_points");
        for (uint32_t i = 0; i < nI && !rc; i++) ok(frog_get_em(c, i, em + 3 * (size_t)i), "frog_get_em");
        uint64_t h = 1469598103934665603ull;
        for (float f : v) { uint32_t b; std::memcpy(&b, &f, 4); h = (h ^ b) * 1099511628211ull; }
        return h;
    }
};
