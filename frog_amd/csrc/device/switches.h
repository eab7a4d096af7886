// switches.h -- the FROG_* environment switches of a device context: read ONCE, when frog_create is
// called, into frog_ctx::sw, and never again -- no getenv on a path a solver step takes (a Python host may change os.environ from
// another thread meanwhile), none cached per process.  Two contexts of one process may differ in every one of them.  Each variable
// keeps the parser it always had (atoi != 0, first character, presence): FROG_CULL_BUILD_PASS=0 still asks for the pass.
// Not here, because they have no context: FROG_ROCTX (a library loaded once per process) and the two *_TRACE_FILE of the trace builds.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace frog {

struct Switches {
    // ---- layout
    bool wide_records = false;      // FROG_WIDE_RECORDS=1 keeps the 8-byte record form where the 4-byte one would fit (test hook)
    // partner groups: 8 (one sweep launch per pass) unless FROG_SUBPASSES asks for 8 * n launches-worth
    // (ctx.h: measured no gain from keeping the slices L2-sized, so it is not automatic)
    int subpasses = 1;
    int tile_slices = 0;            // FROG_TILE_SLICES, 1 .. 64; 0: unset, by the number of owned images (prep.h fused_block_order)
    int fused = -1;                 // FROG_SWEEP_FUSED=0: never the fused sweep; 1: also without a culling list; -1: unset
    // ---- scalar hand-off
    bool scalars_copy = false;      // FROG_SCALARS_COPY: the copy + event hand-off (A/B, fallback)
    // ---- certified outlier culling (k_cull.hip.h): FROG_CULL=0 off; FROG_CULL_SKIN="scale,pad" sets the list cutoff
    bool cull = true;
    bool cull_linear = true;        // the same machinery for the LINEAR stage: on unless FROG_CULL_LINEAR=0
    float cull_scale = 2.0f, cull_pad = 25.0f;          // list cutoff = scale * certified cutoff + pad (the skin)
    float cull_lin_scale = 1.25f, cull_lin_pad = 10.0f; // the linear stage's own skin (the cutoffs are 14.5 c1: far out, where a tighter skin still lasts for iterations)
    bool cull_build_pass = false;   // FROG_CULL_BUILD_PASS: the list by a pass of its own, not by the sweep that walks every record
    // ---- weights
    bool weight_exact = false;      // FROG_WEIGHT_EXACT=1 (test hook): every inlier weight through the form with the reference's own promotions (ten times the arithmetic)
    bool weight_general = false;    // FROG_WEIGHT_GENERAL=1 (test hook): no image gets a range for the one-exponential form
                                    // (k_stats.hip.h em_fast_of with theta = NaN), the deformable sweeps evaluate inlier_probability twice
    // ---- reference order (k_reforder.hip.h, k_refchain.hip.h)
    int reference_order = -1;       // FROG_REFERENCE_ORDER=0 / 1: the tests' switch, overrides frog_options::reference_order; -1: unset
    bool ref_literal = false;       // FROG_REF_LITERAL=1: the literal form (ref_scatter_kernel), for comparison
    uint32_t rc_grid_x = 1u << 22;  // FROG_RC_GRID_X: workgroups in x of the chain kernels' launches (test hook: the fold on small groups)
    bool ref_trace = false;         // FROG_REF_TRACE: host-side times of a lattice's chain build to stderr
    // ---- B-spline transform
    bool k11_f64 = false;           // FROG_K11_F64=1: the B-spline transform's weights and sums in f64 (rounds 1-4), for comparison
    bool k11_pointwise = false, k11_tiled = false;      // FROG_K11_POINTWISE / FROG_K11_TILED force one form (tests)
    int k11_by_xcd = -1;            // FROG_K11_BY_XCD=1 / 0 forces / forbids the brick-order walk (k_grid.hip.h); < 0: by the block count
    int k11_point_by_xcd = -1;      // FROG_K11_POINT_BY_XCD=1 / 0 forces / forbids the XCD-aware order of the blocks; < 0: from 8 192 blocks
    // ---- lattice
    int brick = 0;                  // FROG_BRICK=4 | 8 (test hook): cells per brick edge; 0: by the points per brick (make_geometry)
    int lattice_blocked = -1, lattice_sparse = -1;      // FROG_LATTICE_BLOCKED / FROG_LATTICE_SPARSE = 0 / 1 force a form (A/B, tests); -1: by size
    bool energy_pass = false;       // FROG_ENERGY_PASS: the deformable step's energy reduction as a launch of its own
    // ---- diagnostics
    bool timing = false;            // FROG_TIMING: [timing] lines of the layout build and of frog_create's device part
    // FROG_SETUP_TRACE=1: where the host's time in a lattice set-up goes (a level's first lattice has been seen to take 0.7 s of it on
    // some boxes and 0.016 s on others), and what frog_create reserves for the finest announced level
    bool setup_trace = false;
};

inline Switches read_switches(int max_subpasses)
{
    Switches sw;
    auto on = [](const char *e, bool unset) { return e ? atoi(e) != 0 : unset; };            // "0" = off
    auto tri = [](const char *e) { return e ? (atoi(e) != 0 ? 1 : 0) : -1; };
    auto skin = [](const char *e, float &scale, float &pad) {
        float a = 0, b = 0;
        if (e && sscanf(e, "%f,%f", &a, &b) == 2 && a >= 1.0f && b >= 0.0f) { scale = a; pad = b; }
    };
    const char *e;
    e = getenv("FROG_WIDE_RECORDS"); sw.wide_records = e && e[0] == '1';
    if ((e = getenv("FROG_SUBPASSES"))) sw.subpasses = std::min(max_subpasses, std::max(1, atoi(e)));
    if ((e = getenv("FROG_TILE_SLICES"))) sw.tile_slices = std::min(64, std::max(1, atoi(e)));
    if ((e = getenv("FROG_SWEEP_FUSED"))) sw.fused = e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1;
    sw.scalars_copy = getenv("FROG_SCALARS_COPY") != nullptr;
    sw.cull = on(getenv("FROG_CULL"), true);
    sw.cull_linear = on(getenv("FROG_CULL_LINEAR"), true);
    skin(getenv("FROG_CULL_SKIN"), sw.cull_scale, sw.cull_pad);
    skin(getenv("FROG_CULL_SKIN_LINEAR"), sw.cull_lin_scale, sw.cull_lin_pad);
    sw.cull_build_pass = getenv("FROG_CULL_BUILD_PASS") != nullptr;
    sw.weight_exact = on(getenv("FROG_WEIGHT_EXACT"), false);
    sw.weight_general = on(getenv("FROG_WEIGHT_GENERAL"), false);
    sw.reference_order = tri(getenv("FROG_REFERENCE_ORDER"));
    sw.ref_literal = getenv("FROG_REF_LITERAL") != nullptr;
    if ((e = getenv("FROG_RC_GRID_X"))) sw.rc_grid_x = (uint32_t)std::max(1, atoi(e));
    sw.ref_trace = getenv("FROG_REF_TRACE") != nullptr;
    sw.k11_f64 = on(getenv("FROG_K11_F64"), false);
    sw.k11_pointwise = getenv("FROG_K11_POINTWISE") != nullptr;
    sw.k11_tiled = getenv("FROG_K11_TILED") != nullptr;
    if ((e = getenv("FROG_K11_BY_XCD"))) sw.k11_by_xcd = atoi(e);
    if ((e = getenv("FROG_K11_POINT_BY_XCD"))) sw.k11_point_by_xcd = atoi(e);
    if ((e = getenv("FROG_BRICK"))) { const int b = atoi(e); if (b == 4 || b == 8) sw.brick = b; }
    sw.lattice_blocked = tri(getenv("FROG_LATTICE_BLOCKED"));
    sw.lattice_sparse = tri(getenv("FROG_LATTICE_SPARSE"));
    sw.energy_pass = getenv("FROG_ENERGY_PASS") != nullptr;
    sw.timing = getenv("FROG_TIMING") != nullptr;
    sw.setup_trace = getenv("FROG_SETUP_TRACE") != nullptr;
    return sw;
}

} // namespace frog
