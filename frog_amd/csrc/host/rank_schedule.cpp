// rank_schedule.cpp -- frog_run_schedule (include/frog_host.h): one rank's share of a timed registration schedule, the
// loops of ImageGroup::run (registration/imageGroup.cxx:54-66, :78-128) over the steps of rank_steps.h, between the
// barriers and clocks of the timed region.  No solver arithmetic here.

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/frog_host.h"
#include "rank_steps.h"

namespace frog { void set_last_error(const std::string &s); }      // libfrog_hip.so

namespace {
using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }
} // namespace

extern "C" int frog_run_schedule(frog_ctx *ctx, frog_comm *comm, const frog_schedule_plan *plan, frog_schedule_result *out)
{
    if (!ctx || !plan || !out) { frog::set_last_error("null argument"); return FROG_E_INVALID; }
    if (plan->plan_bytes != sizeof(frog_schedule_plan) || plan->result_bytes != sizeof(frog_schedule_result)) {
        frog::set_last_error("frog_schedule_plan / frog_schedule_result layout differs from the caller's");
        return FROG_E_INVALID;
    }
    if (plan->n_levels < 0 || plan->n_levels > FROG_SCHEDULE_MAX_LEVELS || plan->stat_interval < 1 || plan->warmup_linear < 0 || plan->linear < 0) {
        frog::set_last_error("bad schedule");
        return FROG_E_INVALID;
    }
    std::memset(out, 0, sizeof *out);
    if (comm) {
        std::string err;
        if (!host_comm_api().load(err)) { frog::set_last_error("cannot load libfrog_comm.so: " + err); return FROG_E_INVALID; }
    }
    RankSteps r;
    if (r.init(ctx, comm, plan->proxy_em)) return r.rc;

    auto setup = [&](int level) {
        const auto t0 = clk::now();
        frog_grid_info info{};
        r.setup(level, info);
        if (r.rc || out->n_lattices >= FROG_SCHEDULE_MAX_LATTICES) return;
        frog_schedule_lattice &la = out->lattices[out->n_lattices++];
        la.level = level; la.iterations = 0; la.setup_host_s = since(t0);
        for (int k = 0; k < 3; k++) la.dims[k] = info.dims[k];
    };
    auto barrier = [&] {
        if (r.rc) return;
        if (r.ok(frog_synchronize(ctx), "frog_synchronize")) r.barrier();
    };
    auto phaseEnd = [&](int phase, clk::time_point t0) {
        if (r.rc) return;
        if (plan->profile == 1) {
            if (!r.ok(frog_synchronize(ctx), "frog_synchronize")) return;
            out->phase_s[phase] = since(t0);
            frog_kernel_time kt[FROG_K_COUNT_];
            if (!r.ok(frog_profile_read(ctx, kt, 1), "frog_profile_read")) return;
            for (int k = 0; k < FROG_K_COUNT_; k++) {
                out->kernels_by_phase[phase][k] = kt[k];
                out->kernels[k].ms_total += kt[k].ms_total; out->kernels[k].launches += kt[k].launches;
            }
        } else {
            out->phase_s[phase] = since(t0);
        }
    };

    // ---- untimed: linear set-up, first transform, (proxy: the other ranks' coordinates), warm-up iterations
    const bool trace = getenv("FROG_SCHEDULE_TRACE") != nullptr;
    const auto t_in = clk::now();
    r.ok(frog_linear_init(ctx, plan->anchor), "frog_linear_init");
    if (trace) std::fprintf(stderr, "[schedule] linear_init returned at %.4f s\n", since(t_in));
    r.transformPoints(0);
    if (trace) { frog_synchronize(ctx); std::fprintf(stderr, "[schedule] first transform done at %.4f s\n", since(t_in)); }
    if (!r.rc && plan->proxy_xyz2 && !comm && !r.whole) {
        size_t pb = 0, pe = 0;
        const uint64_t P = frog_num_points(ctx);
        std::vector<float> cur(3 * P);
        r.ok(frog_comm_buffer(ctx, FROG_BUF_XYZ2, nullptr, nullptr, &pb, &pe), "frog_comm_buffer");
        r.ok(frog_get_points(ctx, nullptr, cur.data()), "frog_get_points");
        if (!r.rc) {
            std::memcpy(cur.data(), plan->proxy_xyz2, 3 * pb * sizeof(float));
            std::memcpy(cur.data() + 3 * pe, plan->proxy_xyz2 + 3 * pe, 3 * (P - pe) * sizeof(float));
            r.ok(frog_set_points2(ctx, cur.data()), "frog_set_points2");
        }
    }
    int it = 0;
    double E = 0;
    for (int w = 0; w < plan->warmup_linear && !r.rc; w++, it++) {
        if (it % plan->stat_interval == 0) r.updateStats();
        E = r.linearStep();
        r.transformPoints(0);
    }

    if (trace) { frog_synchronize(ctx); std::fprintf(stderr, "[schedule] warm-up done at %.4f s\n", since(t_in)); }
    // ---- timed region
    r.ok(frog_profile_enable(ctx, plan->profile), "frog_profile_enable");
    if (comm && plan->time_comm) r.ok(r.api->timing(comm, 1), "frog_comm_timing");
    barrier();
    const auto t_start = clk::now();
    auto tp = t_start;
    for (int k = 0; k < plan->linear && !r.rc; k++, it++) {
        if (it % plan->stat_interval == 0) r.updateStats();
        E = r.linearStep();
        r.transformPoints(0);
        out->iterations++;
    }
    r.transformPoints(1);                                       // :70
    phaseEnd(0, tp);
    for (int level = 0; level < plan->n_levels && !r.rc; level++) {
        const int n = plan->per_level[level];
        if (n <= 0) continue;
        tp = clk::now();
        setup(level);                                           // :81
        r.transformPoints(0);
        int grids = 1, diffeo = 0;
        float alpha = plan->deformable_alpha;
        for (int iteration = 0; iteration < n && !r.rc; iteration++) {
            if (iteration % plan->stat_interval == 0) r.updateStats();
            const double e = r.deformableStep(alpha, iteration + 1 < n && (iteration + 1) % plan->stat_interval != 0);
            if (r.rc) break;
            if ((float)e < 0) {                                 // :97-115
                if (diffeo == 0) alpha /= 2;
                grids++;
                iteration--;
                r.transformPoints(1);
                setup(level);
                r.transformPoints(0);
                diffeo = 0;
                continue;
            }
            diffeo++;
            r.transformPoints(0);
            E = e;
            out->iterations++;
            if (out->n_lattices > 0) out->lattices[out->n_lattices - 1].iterations++;
        }
        out->grids_per_level[level] = grids;
        r.transformPoints(1);                                   // :126
        phaseEnd(1 + level, tp);
    }
    barrier();
    out->elapsed_s = since(t_start);
    if (trace) std::fprintf(stderr, "[schedule] timed region %.4f s, ends at %.4f s\n", out->elapsed_s, since(t_in));
    out->final_E = (double)(float)E;
    if (r.rc) return r.rc;

    // ---- after the timed region: kernel and collective times, the replica's hash
    if (plan->profile != 1) r.ok(frog_profile_read(ctx, out->kernels, 1), "frog_profile_read");
    r.ok(frog_profile_enable(ctx, 0), "frog_profile_enable");
    if (comm && plan->time_comm) {
        r.ok(r.api->timing_read(comm, out->comm_ms, out->comm_calls, out->comm_sampled), "frog_comm_timing_read");
        r.ok(r.api->timing(comm, 0), "frog_comm_timing");
    }
    if (plan->n_levels == 0) r.transformPoints(1);      // linear only: leave re-based coordinates, as the levels do
    if (r.rc) return r.rc;
    out->replica_hash = r.replicaHash();
    return r.rc;
}
