"""Round 6: (1) the product path against reference-order mode over cfg 3's WHOLE default schedule inside the suite (VERDICT r5
item 1), with the form of the B-spline transform that moved the raw coefficients named by a test; (2) reference-order mode's
fast kernels (one chain per control point, rows of half-links side by side, a producer / consumer linear chain) against the
literal forms of rounds 4-5, bit for bit."""
import numpy as np
import pytest

from frog_amd import schedule
from frog_amd.pairs import Pairs
from gpu_util import Side, _frog, _same_files, fast_against_reference_order, ragged_pairs, report

pytestmark = pytest.mark.gpu


# ---- (1) product path vs reference-order mode, cfg 3, -li 50 -dl 3 -di 200 ------------------------------------------------------
# Bisected in round 6 (profiles/r06_parity_bisect.txt): of round 5's two arithmetic
# changes the scatter's fused multiply-add moves NOTHING (cells fma / two roundings agree to three digits on every lattice), the
# f32 form of the B-spline transform (K11) moves the raw coefficients of ONE rim node (second level-2 lattice, image 45 node 6037:
# support 5.7e-8 from a single point, node weight 1.9e-20) from 2.0e-4 to 4.2e-3 of max|c| and the whole chain on a dense lattice
# from 6.0e-7 to 3.0e-6.  The f64 form costs 5 % of the 650-step line (0.056 / 0.057 / 0.085 against 0.037 / 0.040 / 0.062 ms per
# launch), so the f32 form stays the default and its bars are the measured values x 3; FROG_K11_F64=1 holds round 4's bars.
BARS = {
    #        raw      dense   field   weighted  chain   E
    "f32": (1.3e-2, 1.0e-4, 1.0e-4, 1.5e-5, 1.0e-5, 1e-6),      # measured 4.2e-3, 3.3e-5, 3.4e-5, 5.0e-6, 3.0e-6, 7.0e-8
    "f64": (1.0e-3, 1.0e-4, 1.0e-4, 1.5e-5, 2.0e-6, 1e-6),      # measured 2.0e-4, 1.4e-5, 2.8e-5, 3.9e-6, 6.0e-7, 7.0e-8
}


@pytest.mark.parametrize("k11", ["f32", "f64"])
def test_fast_path_against_reference_order_config3_whole_default_schedule(monkeypatch, k11):
    """BASELINE.json configs[2] at its size over the reference's whole default schedule: 650 accepted iterations, 65 refreshes,
    the guard's rejections (1 / 2 / 4 lattices per level).  Same guard decisions (frog_amd.schedule asserts them at every step), census
    equal, and per lattice the bars above -- a ten-fold regression of any of them fails here, not in a script."""
    monkeypatch.setenv("FROG_K11_F64", "1" if k11 == "f64" else "0")
    pairs = Pairs.synthetic(100, 20000, 10101, seed=1)
    r = fast_against_reference_order(pairs, 50, 3, 200, monkeypatch, range(0, 100, 9))
    report(f"fast_vs_reference_order_cfg3_whole_schedule_{k11}", r)
    raw, dense, field, weighted, chain, e = BARS[k11]
    assert r["grids"] == [1, 2, 4]
    for k, d in enumerate(r["lattices"]):
        assert d["raw"] <= raw and d["dense_field"] <= dense and d["field"] <= field and d["weighted"] <= weighted, (k, d)
    assert r["E"] < e and r["matrices"] < 1e-6 and r["xyz"] < 1e-6 and r["chain"]["rel"] <= chain
    assert r["census"] == 0            # the two runs' final inlier census, half-link for half-link (equal in every run so far)


# ---- (2) reference-order mode: the fast forms against the literal ones ------------------------------------------------------------

def run_reference_order(pairs, monkeypatch, li, dl, di, images, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FROG_REFERENCE_ORDER", "1")
    s = Side(pairs)
    monkeypatch.delenv("FROG_REFERENCE_ORDER")
    for k in env:
        monkeypatch.delenv(k)
    trace = []

    def check(tag, sides, e=None, infos=None):
        kind = schedule.kind(tag)
        if kind == "step":
            info = s.grid(images[0], s.num_grids() - 1)[0]
            n_cp = info.dims[0] * info.dims[1] * info.dims[2]
            trace.append(("sums", s.point_sums().copy()))
            trace.append(("grad", np.stack([s.gradient_raw(i, n_cp) for i in images])))
        elif kind in ("linear", "deformable"):
            trace.append((kind, s.xyz2().copy(), s.matrices().copy(), float(e[0])))
    grids = schedule.run([s], li, [di] * dl, on=check)
    trace.append(("final", s.xyz2().copy(), s.matrices().copy()))
    lattices = [np.stack([s.grid(i, k)[1] for i in images]) for k in range(s.num_grids())]
    return grids, trace, lattices


def same_trace(a, b):
    assert a[0] == b[0]
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert x[0] == y[0]
        for u, v in zip(x[1:], y[1:]):
            assert np.array_equal(u, v), x[0]
    for u, v in zip(a[2], b[2]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("group", ["small", "ragged", "cfg5_shaped"])
def test_reference_order_fast_forms_equal_the_literal_forms(monkeypatch, group):
    """bin/frog -exact 1 with its round-6 kernels (k_refchain.hip.h: one chain per control point; the rows of half-links side by
    side; the linear chain fed by producer wavefronts) against FROG_REF_LITERAL=1 (ref_scatter_kernel, one wavefront per image
    with a barrier per point; a thread per point over the reference-order CSR; terms and chain in two kernels): per-point sums,
    gradient images, coordinates, matrices, energies and every lattice bit for bit, free-running with regrids."""
    if group == "small":
        pairs, sched, images = Pairs.synthetic(6, 3000, 1500, seed=7), (12, 3, 25), list(range(6))
    elif group == "ragged":
        pairs = ragged_pairs()
        sched, images = (8, 2, 6), list(range(pairs.n_images))
    else:
        pairs, sched, images = Pairs.synthetic(40, 20000, 16667, seed=2, partners_per_image=20), (4, 5, 2), list(range(0, 40, 7))
    fast = run_reference_order(pairs, monkeypatch, *sched, images)
    literal = run_reference_order(pairs, monkeypatch, *sched, images, FROG_REF_LITERAL="1")
    same_trace(fast, literal)


def test_reference_order_chain_launches_folded_into_two_grid_dimensions(monkeypatch):
    """rc_grid() with at most 5 workgroups in x (FROG_RC_GRID_X=5, a switch of the context like every other): the fill's and the
    chain kernel's groups come from blockIdx.z / .y * gridDim.x + blockIdx.x with a bound check, as on cfg 5's finest lattice
    where the fold is needed -- same per-step sums, gradients, energies, coordinates, matrices and lattices as the unfolded
    launch.  The folded context is the SECOND of the process: a cap that the first context fixed for everyone would test nothing."""
    monkeypatch.delenv("FROG_RC_GRID_X", raising=False)
    pairs, images = Pairs.synthetic(6, 3000, 1500, seed=7), list(range(6))
    plain = run_reference_order(pairs, monkeypatch, 6, 3, 8, images)
    folded = run_reference_order(pairs, monkeypatch, 6, 3, 8, images, FROG_RC_GRID_X="5")
    assert len(plain[2]) >= 3 and plain[1][-1][0] == "final"      # with the final coordinates and matrices: five arrays or more
    same_trace(plain, folded)


def test_reference_order_fast_forms_equal_the_literal_forms_at_config5_size(monkeypatch):
    """The same at BASELINE.json configs[4]'s size, -li 2 -dl 5 -di 1: its finest lattice has 5.5e8 (image, control point) pairs =
    3.4e7 groups of chains, and a launch of one 256-thread workgroup per group is 8.8e9 work-items in x -- more than the 32-bit
    grid of a dispatch packet.  The launch reported no error and left the groups past 2^24 unfilled (found at full size by
    scripts/diag_exact_forms.py; the 40-image group above cannot see it).  rc_grid() folds the groups into two grid dimensions."""
    pairs = Pairs.synthetic(500, 20000, 16667, seed=1, partners_per_image=60)
    images = list(range(0, 500, 71))
    fast = run_reference_order(pairs, monkeypatch, 2, 5, 1, images)
    literal = run_reference_order(pairs, monkeypatch, 2, 5, 1, images, FROG_REF_LITERAL="1")
    assert fast[0] == [1, 1, 1, 1, 1]
    same_trace(fast, literal)


# ---- (3) two collectives per iteration without a device-visible scalar block -----------------------------------------

def test_two_collectives_flow_with_the_scalars_by_copy(tmp_path):
    """FROG_SCALARS_COPY=1 = the state a failed hipHostGetDevicePointer leaves: frog_comm_unpack_slab_step used to return
    FROG_E_STATE there, i.e. every multi-rank run aborted at its first linear iteration.  Now the summed scalars reach the host by
    hipMemcpyAsync + event and frog_step_finish waits for the event: same files as the default hand-off, rejections included."""
    pairs = Pairs.synthetic(9, 3000, 1200, seed=4)
    direct, copy = tmp_path / "direct", tmp_path / "copy"
    for d in (direct, copy):
        d.mkdir()
        pairs.write(d / "pairs.bin")
    flags = ("-ngl", "3", "-gm", "0.004")
    out = _frog(direct, *flags)
    _frog(copy, *flags, env_extra={"FROG_SCALARS_COPY": "1"})
    assert out.count("Iteration canceled") >= 2
    _same_files(direct, copy, pairs.n_images)


def test_one_context_with_the_scalars_by_copy_and_rejected_steps(tmp_path):
    """The same fallback in ONE context: frog_deformable_phase_c then gets the step's scalars by hipMemcpyAsync + event instead of
    from the transform queued behind the step.  With -gm 0.004 the guard rejects steps either way: same files, same rejections."""
    pairs = Pairs.synthetic(9, 3000, 1200, seed=4)
    direct, copy = tmp_path / "direct", tmp_path / "copy"
    for d in (direct, copy):
        d.mkdir()
        pairs.write(d / "pairs.bin")
    flags = ("-gm", "0.004")
    out_direct = _frog(direct, *flags)
    out_copy = _frog(copy, *flags, env_extra={"FROG_SCALARS_COPY": "1"})
    assert out_direct.count("Iteration canceled") >= 2 and out_copy.count("Iteration canceled") >= 2
    _same_files(direct, copy, pairs.n_images)


# ---- (4) fine lattices of many images: blocks of 16 nodes across the images, entries for active pairs only (k_grid.hip.h) ------------

@pytest.mark.parametrize("flags", [(), ("-ngl", "3"), ("-gm", "0.004")])
@pytest.mark.parametrize("forms", [{"FROG_LATTICE_BLOCKED": "1"}, {"FROG_LATTICE_SPARSE": "1"}, {"FROG_LATTICE_BLOCKED": "1", "FROG_LATTICE_SPARSE": "1"}])
def test_blocked_and_sparse_lattices_give_the_same_files(tmp_path, flags, forms):
    """The two forms lattices of >= 2^27 (image, node) pairs get by themselves (cfg 5's finest level), forced on a group that would
    never choose them, against the plain form: FROG_LATTICE_BLOCKED=1 ([node / 16][image][node % 16] instead of image-major: moves
    entries, no arithmetic) and FROG_LATTICE_SPARSE=1 (entries for the pairs some point of the image reaches; every other pair of a
    node holds the same float -- 0 minus the node's means so far -- kept once per node).  Identical measures.csv and transforms for
    one context, three sharded contexts (phase B by cp_center_kernel, the speculative third lattice and its companion) and a run whose
    guard rejects steps (retired lattices read back through their own layout, mask and shared values)."""
    pairs = Pairs.synthetic(9, 3000, 1200, seed=4)
    plain, other = tmp_path / "plain", tmp_path / "other"
    for d in (plain, other):
        d.mkdir()
        pairs.write(d / "pairs.bin")
    _frog(plain, *flags, env_extra={"FROG_LATTICE_BLOCKED": "0", "FROG_LATTICE_SPARSE": "0"})
    _frog(other, *flags, env_extra={"FROG_LATTICE_BLOCKED": "0", "FROG_LATTICE_SPARSE": "0", **forms})
    _same_files(plain, other, pairs.n_images)


@pytest.mark.parametrize("flags", [(), ("-ngl", "3"), ("-gm", "0.004")])
def test_xcd_order_of_the_transform_blocks_changes_no_bit(tmp_path, flags):
    """The B-spline transform deals its blocks to the XCDs by image on fine lattices (the tiled form walks
    the block table in brick order, an eighth per XCD, from 16 384 blocks; the thread-per-point form its 256-point blocks, from
    8 192).  A block computes what it computed before, only elsewhere and at another time: both orders forced on a group that would
    never choose them, in both forms of the transform, against both forbidden -- identical measures.csv and transforms, for one
    context, three sharded contexts and a run whose guard rejects steps (the per-block displacement maxima of the culling list are
    written under the new block numbers)."""
    pairs = Pairs.synthetic(9, 3000, 1200, seed=4)
    runs = {"tiled_plain": {"FROG_K11_TILED": "1", "FROG_K11_BY_XCD": "0"}, "tiled_xcd": {"FROG_K11_TILED": "1", "FROG_K11_BY_XCD": "1"},
            "point_plain": {"FROG_K11_POINTWISE": "1", "FROG_K11_POINT_BY_XCD": "0"}, "point_xcd": {"FROG_K11_POINTWISE": "1", "FROG_K11_POINT_BY_XCD": "1"}}
    for name, env in runs.items():
        d = tmp_path / name
        d.mkdir()
        pairs.write(d / "pairs.bin")
        _frog(d, *flags, env_extra=env)
    for name in ("tiled_xcd", "point_plain", "point_xcd"):
        _same_files(tmp_path / "tiled_plain", tmp_path / name, pairs.n_images)


# ---- (5) the scatter's hand-scheduled DPP statement against the plain form ---------------------------------------------

def test_scatter_quad_form_equals_the_point_by_point_form_bit_for_bit(tmp_path):
    """The scatter's phase 2 reads four points' weights per LDS instruction and hands the sums round the quad with v_fmac_f32_dpp
    inside an asm statement (k_grid.hip.h FROG_FMAC4_DPP: the compiler's hazard recogniser does not look inside).  Against a build
    without it (`make variants`: -DFROG_SCATTER_QUADS=0, frog_amd/lib/variants/libfrog_hip_noquads.so): the same schedule in two
    processes, coordinates, energies and every lattice identical."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    variant = os.path.join(os.path.dirname(here), "frog_amd", "lib", "variants", "libfrog_hip_noquads.so")
    if not os.path.exists(variant):
        pytest.skip("frog_amd/lib/variants/libfrog_hip_noquads.so not built (make -C frog_amd/csrc variants)")
    outs = []
    for lib in (None, "variants/libfrog_hip_noquads.so"):
        env = dict(os.environ)
        env.pop("FROG_HIP_LIB", None)
        if lib:
            env["FROG_HIP_LIB"] = lib
        out = tmp_path / ("quads.npz" if lib is None else "plain.npz")
        r = subprocess.run([sys.executable, os.path.join(here, "run_lattices.py"), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(np.load(out))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 6
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k


# ---- (6) the ahead-of-time selections beside the first iterations (frog_options::selections_in_background) ------------------------

def test_selections_in_background_change_nothing(monkeypatch):
    """bin/frog creates its context with selections_in_background = 1: frog_create queues the reservoir selections of the first
    refreshes on the side stream and returns without waiting; a refresh waits for its own selection's event.  The same schedule
    with and without: coordinates, matrices, mixtures and every lattice bit for bit (13 refreshes over three levels)."""
    pairs = Pairs.synthetic(12, 4000, 1500, seed=5)
    out = []
    for flag in (0, 1):
        s = Side(pairs, selections_in_background=flag)
        grids = schedule.run([s], 30, [30] * 3)
        out.append((grids, s.xyz2().copy(), s.matrices().copy(), np.stack([s.g.em(i) for i in range(pairs.n_images)]),
                    [np.stack([s.grid(i, k)[1] for i in range(pairs.n_images)]) for k in range(s.num_grids())]))
    a, b = out
    assert a[0] == b[0]
    for u, v in zip(a[1:4], b[1:4]):
        assert np.array_equal(u, v)
    for u, v in zip(a[4], b[4]):
        assert np.array_equal(u, v)


# ---- (7) the finest level's buffers reserved at frog_create (frog_options::max_levels_hint) ------------------------------------------

def test_no_lattice_allocation_after_create_when_the_levels_are_announced():
    """A cfg-5-shaped group (40 images lying +-100 mm apart, five levels): with max_levels_hint = 5 frog_create sizes the lattice
    buffers for the fifth level from the per-image boxes centred on one point -- what the linear initialisation makes of them --
    and no set-up allocates afterwards.  Round 6 found the estimate taken from the boxes where they lie: 3.8 times too large
    at cfg 5's size, refused as more than half of the device's memory, and the set-up of level 4 paid three hipMalloc of 7.4 GB
    inside the loops (17 to 1 230 ms, box to box).  Without the hint the set-ups allocate: the counter counts."""
    pairs = Pairs.synthetic(40, 20000, 16667, seed=2, partners_per_image=20)
    hinted = Side(pairs, max_levels_hint=5)
    schedule.run([hinted], 4, [2] * 5)
    assert hinted.g.lattice_reallocations() == 0
    plain = Side(pairs)
    schedule.run([plain], 4, [2] * 5)
    assert plain.g.lattice_reallocations() >= 1
