"""EULER_PRECOND_IC0_TILE on the GPU (k_factor_tile, k_precond_tile; k_sweep_simple as the second schedule) against the oracle's restatement of the same
blocks (oracle eo_tile_start): bit-exact in EULER_DOT_SEQUENTIAL - each block's recurrences have no reduction - and, against
the REFERENCE's IC(0), tolerance parity where PCG converges (the mode changes the iterates, not the solution)."""
import numpy as np
import pytest

import euler_amd as ea
from golden_util import load, scenario_text
from oracle_lib import Oracle
from resident_ref import random_scene_text
from test_gpu_parity import assert_bits, compare_all

pytestmark = pytest.mark.gpu

TILE_SHAPES = [((144, 100), 16), ((400, 130), 8), ((400, 130), 32), ((1024, 200), 16), ((1024, 200), 32), ((1025, 130), 8),
               ((65, 300), 16), ((2000, 70), 16), ((333, 127), 32)]


@pytest.mark.parametrize("sweep", [ea.SWEEP_BAND, ea.SWEEP_SIMPLE])
@pytest.mark.parametrize("shape,units", TILE_SHAPES)
def test_tile_sweeps_random_masks_bit_exact(shape, units, sweep):
    """Factor (stale entries of non-fluid neighbours inside a block included), forward and backward solve of the tile-local
    mode on random fluid / solid patterns; widths of one and of many tiles, partial top band, both schedules."""
    X2, Y2 = shape
    rng = np.random.default_rng(X2 * 1000 + Y2 + units)
    count = np.zeros((Y2, X2), np.uint8)
    solid = np.zeros((Y2, X2), np.uint8)
    inner = (slice(1, Y2 - 1), slice(1, X2 - 1))
    count[inner] = (rng.random((Y2 - 2, X2 - 2)) < 0.7) * rng.integers(1, 5, (Y2 - 2, X2 - 2))
    solid[inner] = rng.random((Y2 - 2, X2 - 2)) < 0.1
    count[solid > 0] = 0
    if X2 > 600:
        count[:, 300:520] = 0          # whole tiles without fluid: skipped by every sweep
    sink = np.zeros((Y2, X2), np.uint8)
    sink[0, :] = sink[-1, :] = sink[:, 0] = sink[:, -1] = 1
    stale = rng.random((Y2, X2)) * (rng.random((Y2, X2)) < 0.5)
    fluid = count > 0
    r = np.where(fluid, rng.standard_normal((Y2, X2)), 0.0)
    zero_f = np.zeros((Y2, X2), np.float32)

    o = Oracle(X2, Y2)
    o.c.tile_records = units
    o.count[...] = count; o.solid[...] = solid; o.sink[...] = sink
    o.precon[...] = stale
    o.lib.eo_build_system(o.ptr, np.float32(0.1), o.f32p(o.utmp), o.f32p(o.vtmp))
    o.r[...] = r
    o.lib.eo_apply_preconditioner(o.ptr, o.f64p(o.r), o.f64p(o.z))

    sim = ea.Simulation(X2, Y2, dot_mode=ea.DOT_SEQUENTIAL, sweep_mode=sweep, precond=ea.PRECOND_IC0_TILE, tile_records=units)
    for f, a in ((ea.F_SOLID, solid), (ea.F_SOURCE, np.zeros_like(solid)), (ea.F_SINK, sink), (ea.F_COUNT, count),
                 (ea.F_PREV_COUNT, count), (ea.F_UTMP, zero_f), (ea.F_VTMP, zero_f), (ea.F_PRECON, stale)):
        sim.set(f, a)
    sim.set_markers(np.zeros((0, 2), np.float32))
    sim.pcg_op(ea.OP_BUILD_SYSTEM, 0.1)
    sim.set(ea.F_PCG_R, r)
    for rep in range(2):
        sim.pcg_op(ea.OP_PRECON_FACTOR)
        assert_bits(sim.get(ea.F_PRECON), o.precon, "precon %s rep %d" % (shape, rep), nan_class=True)
        sim.pcg_op(ea.OP_FORWARD_SOLVE)     # a no-op in the fused schedule: q never leaves the registers there
        if sweep == ea.SWEEP_SIMPLE:
            assert_bits(sim.get(ea.F_PCG_Q), o.q, "q %s" % (shape,), nan_class=True)
        sim.pcg_op(ea.OP_BACKWARD_SOLVE)    # fused schedule: the whole Z = M^-1 R
        assert_bits(sim.get(ea.F_PCG_Z), o.z, "z %s" % (shape,), nan_class=True)
        o.lib.eo_apply_preconditioner(o.ptr, o.f64p(o.r), o.f64p(o.z))


@pytest.mark.parametrize("size,scn,units,frames", [((320, 192), "weird-edges", 16, 6), ((512, 256), "block", 32, 4),
                                                   ((257, 129), "filter", 8, 8), ((130, 70), "block", 16, 12),
                                                   ((192, 200), "waterfall", 16, 10)])
def test_tile_mode_free_running_bit_exact_vs_oracle(size, scn, units, frames):
    text = scenario_text(load(scn + "_frames.npz"))
    o = Oracle(size[0], size[1]).load_text(text, upscale=True)
    o.c.tile_records = units
    sim = ea.Simulation(size[0], size[1], dot_mode=ea.DOT_SEQUENTIAL, precond=ea.PRECOND_IC0_TILE, tile_records=units).load_text(text, upscale=True)
    for f in range(frames):
        o.step()
        sim.step()
        st = sim.stats()
        assert st.last_substeps == o.c.last_substeps and st.last_pcg_iterations == o.c.last_pcg_iterations, f
        compare_all(o, sim, "%s %s frame %d" % (scn, size, f))


def test_tile_mode_reaches_the_reference_pressure_where_pcg_converges():
    """Against the REFERENCE's preconditioner (oracle, exact IC(0)): 256x256 half tank, tolerance 1e-6, enough iterations
    for both: |dp| <= 1e-5 max|p|, identical cell grids, velocities within 1e-5; iteration counts printed (-s)."""
    o = Oracle(256, 256).load_half_tank()
    o.c.max_iterations = 3000
    sim = ea.Simulation(256, 256, dot_mode=ea.DOT_SEQUENTIAL, precond=ea.PRECOND_IC0_TILE, tile_records=16, max_iterations=3000).load_half_tank()
    for f in range(2):
        o.step()
        sim.step()
    st = sim.stats()
    print("iterations to 1e-6: reference IC(0) %d, tile-local (64 x 16 blocks) %d" % (o.c.total_pcg_iterations, st.total_pcg_iterations))
    assert st.last_residual <= 1e-6 and o.c.last_residual <= 1e-6
    p, pr = sim.get(ea.F_PRESSURE), o.p
    assert np.abs(p - pr).max() <= 1e-5 * np.abs(pr).max()
    assert_bits(sim.get(ea.F_COUNT) > 0, o.count > 0, "fluid/air grid")
    assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-5 and np.abs(sim.get(ea.F_V) - o.v).max() < 1e-5
    assert st.total_pcg_iterations <= 1.6 * o.c.total_pcg_iterations


def oracle_from_sim(sim, tile_records=0):
    """An oracle holding exactly the state of a GPU handle (everything sim_step depends on, g_precon included)."""
    o = Oracle(sim.X, sim.Y)
    o.c.tile_records = tile_records
    for f, n in ((ea.F_U, "u"), (ea.F_V, "v"), (ea.F_UTMP, "utmp"), (ea.F_VTMP, "vtmp"), (ea.F_SOLID, "solid"), (ea.F_SOURCE, "source"),
                 (ea.F_SINK, "sink"), (ea.F_COUNT, "count"), (ea.F_PREV_COUNT, "prev_count"), (ea.F_PRECON, "precon")):
        getattr(o, n)[...] = sim.get(f)
    o.set_markers(sim.get(ea.F_MARKERS))
    st = sim.stats()
    o.c.rng_state = st.rng_state
    o.c.source_exhausted = st.source_exhausted
    return o


@pytest.mark.parametrize("precond,units", [(ea.PRECOND_IC0_TILE, 16), (ea.PRECOND_IC0, 0)])
def test_tree_dot_1024_dam_break_expensive_phase_vs_oracle(precond, units):
    """The production configuration at BASELINE configs[1]'s size: EULER_DOT_TREE (the default above 65 536 cells) at 1024^2,
    dam break, in the EXPENSIVE phase (every substep runs PCG to the 100-iteration cap), both preconditioner modes.  The GPU
    rolls to the first such frame (the free fall before it involves no dot product at all), the oracle takes over that state
    (teacher forcing) and both run the next frame: 4-8 substeps x 100 iterations.  Only the dot products round differently:
    cell grid and marker count identical, |du|,|dv| <= 1e-6 (float velocities of magnitude ~10), |dp| <= 1e-7 max|p|."""
    text = scenario_text(load("block_frames.npz"))
    sim = ea.Simulation(1024, 1024, dot_mode=ea.DOT_TREE, precond=precond, tile_records=units).load_text(text, upscale=True)
    for _ in range(60):
        sim.step()
        if sim.stats().last_pcg_iterations >= 100:
            break
    assert sim.stats().last_pcg_iterations >= 100
    o = oracle_from_sim(sim, units)
    o.step()
    sim.step()
    st = sim.stats()
    print("substeps %d / %d, iterations %d / %d" % (st.last_substeps, o.c.last_substeps, st.last_pcg_iterations, o.c.last_pcg_iterations))
    # a solve that converges just at the tolerance may stop one iteration earlier or later when the dot products round differently
    assert st.last_substeps == o.c.last_substeps and abs(st.last_pcg_iterations - o.c.last_pcg_iterations) <= 2 * st.last_substeps
    assert o.c.last_pcg_iterations >= 100
    assert_bits(sim.get(ea.F_COUNT), o.count, "count")
    assert st.n_markers == o.n_markers
    pr = o.p
    dp = np.abs(sim.get(ea.F_PRESSURE) - pr).max() / np.abs(pr).max()
    du, dv = np.abs(sim.get(ea.F_U) - o.u).max(), np.abs(sim.get(ea.F_V) - o.v).max()
    print("1024^2 dam break, tree dot, precond %d: %d substeps, %d iterations; |dp|/max|p| %.3e |du| %.3e |dv| %.3e"
          % (precond, st.last_substeps, st.last_pcg_iterations, dp, du, dv))
    assert dp <= 1e-7 and du <= 1e-6 and dv <= 1e-6


def test_switching_the_preconditioner_on_a_live_handle():
    """euler_set_precond: exact IC(0) -> tile-local -> exact on one handle equals fresh handles of each mode (g_precon is
    rewritten on every fluid cell by each factorisation; stale non-fluid entries are shared state)."""
    text = scenario_text(load("block_frames.npz"))
    a = ea.Simulation(300, 200, dot_mode=ea.DOT_SEQUENTIAL).load_text(text, upscale=True)
    o = Oracle(300, 200).load_text(text, upscale=True)
    for units in (0, 16, 0):
        a.set_precond(ea.PRECOND_IC0_TILE if units else ea.PRECOND_IC0, units)
        o.c.tile_records = units
        for _ in range(3):
            a.step()
            o.step()
        compare_all(o, a, "units %d" % units)


@pytest.mark.parametrize("max_it", [100, 37, 2, 1])
def test_interior_chunks_and_two_step_pressure_update_bit_exact(max_it):
    """Chunks deep inside the water (every cell fluid, four fluid neighbours, a_diag 4) take the constant-mask instantiations of
    k_search_apply / k_precond_tile with E^-1 from the per-handle table (k_tile_table) instead of the precon array, and p is
    updated every second iteration with the two fmadds that are due (k_search_apply PMODE 2, k_finish_p): budgets that end on an
    even and on an odd iteration, one and two iterations, against the oracle's plain restatement - every bit of p, u, v."""
    X, Y = 260, 300      # band 1 (rows 64..127) lies whole inside the half tank's water: interior tiles at records 80..255
    o = Oracle(X, Y).load_half_tank()
    o.c.tile_records = 16
    o.c.max_iterations = max_it
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL, precond=ea.PRECOND_IC0_TILE, tile_records=16, max_iterations=max_it).load_half_tank()
    for f in range(3):
        o.step()
        sim.step()
        st = sim.stats()
        assert st.last_substeps == o.c.last_substeps and st.last_pcg_iterations == o.c.last_pcg_iterations, f
        compare_all(o, sim, "half tank %dx%d, budget %d, frame %d" % (X, Y, max_it, f))
    m = sim.get(ea.F_CELLMASK)
    assert (m[64:128, 3:257] == 0x9F).all()      # the band really is interior


def test_tile_mode_moving_water_lean_assembly_bit_exact():
    """A dam break several bands deep, 30 frames in tile-local mode: chunks turn from interior to partial to empty and back while
    the assembly (k_build_system<true>) only rewrites the chunks that hold or held fluid - against the oracle every frame, and
    the solver's own arrays must carry no stale entry: masks and p are +0 wherever the cell grid says air."""
    text = scenario_text(load("block_frames.npz"))
    X, Y = 384, 448
    from trajectories import oracle_for
    o = oracle_for("lean_384x448")      # (the oracle with tile_records = 16 on this scenario; recorded: tests/trajectories.py)
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL, precond=ea.PRECOND_IC0_TILE, tile_records=16).load_text(text, upscale=True)
    for f in range(30):
        o.step()
        sim.step()
        compare_all(o, sim, "dam break %dx%d frame %d" % (X, Y, f))
        air = sim.get(ea.F_COUNT) == 0
        assert (sim.get(ea.F_CELLMASK)[air] == 0).all(), f
        assert (sim.get(ea.F_PRESSURE)[air] == 0).all(), f


def test_tile_mode_fields_against_the_reference_preconditioner_per_baseline_workload():
    """What the roofline mode's FIELDS are worth against the reference's IC(0), from one state per BASELINE
    workload, one frame each: tile-local mode on the GPU, the reference's preconditioner on the oracle (bench.py's
    parity_vs_reference block, the same code).

    * Where the solves converge inside the reference's budget of 100 iterations (main.c:735) the two agree to solver tolerance:
      first solving frame of the 1024^2 dam break - |du|, |dv| <= 1e-5, identical cell grid and marker count.
    * Where the cap cuts the solves short - every BASELINE workload at its size once real pressures build up - both answers are
      unconverged and they differ by what the missing iterations would still have moved: parity with the reference's fields
      does NOT hold there, by design of the cap, and this test says so explicitly: it records the deviation, checks that it is an
      unconverged-solve effect (the structural state - cell grid, marker count - still agrees to 1e-4 of the fluid cells after the
      frame), and that the reference's residual is within reach of the tile-local mode at a profit: on the next system of the
      same state a scan finds the iteration budget at which the tile-local solve is at or below the residual the reference's
      IC(0) reaches in 100 (measured: 144 ... 484, the inf-norm residual of CG oscillates), and the solve with that budget still
      ends sooner than the reference's 100 iterations (measured 1.6x ... 3.4x)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from euler_amd import scenarios
    from oracle_lib import build_oracle
    # (bench.py --quality runs the half tank at 2048^2; here at 1024^2 - a quarter of the oracle's time, the same assertions)
    cases = bench.PARITY_CASES[:2] + (("1024x1024 half tank from rest (configs[2] at 1/64 of its cells)", 1024, "half_tank", 0, 0),) + bench.PARITY_CASES[3:]
    res = bench.parity_vs_reference(ea, scenarios, build_oracle(), 0, ea.DOT_TREE, 0, cases=cases)
    assert len(res) == 4
    converged = [e for e in res if not e["capped"]]
    capped = [e for e in res if e["capped"]]
    assert converged and capped
    for e in res:
        print(e)
        assert e["markers"][0] == e["markers"][1]
        assert e["fluid_cells_differing"] <= 1e-4 * e["fluid_cells"] + 2
    for e in converged:
        assert e["max_abs_du"] <= 1e-5 and e["max_abs_dv"] <= 1e-5 and e["fluid_cells_differing"] == 0, e
    for e in capped:
        ns = e["next_system"]
        assert "error" not in ns, ns
        if ns["residual_reference_ic0_100"] > 0 and e["max_p"] > 0:
            assert ns["tile_budget_for_equal_residual"] is not None and ns["tile_budget_for_equal_residual"] <= 1200, ns
            assert ns["solve_speedup_at_equal_residual"] >= 1.2, ns
    # ... and against the CONVERGED frame of the same state (multilevel mode, cap lifted): the recorded distances of the three capped runs
    for e in res:
        ac = e["against_converged"]
        assert "error" not in ac, ac
        assert ac["converged"]["residual_last_solve"] <= 1e-6
        print(e["state"], {k: v for k, v in ac.items()})
    for e in converged:      # where the reference's cap does not bind, everybody sits on the converged frame
        ac = e["against_converged"]
        for k in ("reference_ic0_cap_100", "tile_local_cap_100", "multilevel_cap_100"):
            assert ac[k]["max_abs_du"] <= 1e-4 and ac[k]["max_abs_dv"] <= 1e-4, (k, ac)
    for e in capped:         # where it binds, the multilevel mode at the same cap is the nearest of the three (the half tank: by orders of magnitude)
        ac = e["against_converged"]
        if e["max_p"] > 0 and e["max_abs_velocity"] > 0:
            m, r, t = (max(ac[k]["max_abs_du"], ac[k]["max_abs_dv"]) for k in ("multilevel_cap_100", "reference_ic0_cap_100", "tile_local_cap_100"))
            assert m <= r * 1.05 + 1e-6 and m <= t * 1.05 + 1e-6, ac


# ----------------------------------------------------------------------------- two-level preconditioner (EULER_PRECOND_IC0_TILE2)
def _two_level_pair(X, Y, max_it, text=None, mg=False):
    o = Oracle(X, Y)
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG if mg else ea.PRECOND_IC0_TILE2, tile_records=16, max_iterations=max_it)
    if text is None:
        o.load_half_tank(); sim.load_half_tank()
    else:
        o.load_text(text, upscale=True); sim.load_text(text, upscale=True)
    o.c.tile_records = 16
    o.c.coarse_m = o.lib.eo_coarse_m(X, Y)
    o.c.coarse_mg = int(mg)
    o.c.max_iterations = max_it
    return o, sim


@pytest.mark.parametrize("X,Y", [(260, 300), (1100, 200), (130, 1030)])
def test_two_level_preconditioner_matches_the_oracle_restatement(X, Y):
    """z = M_tile^-1 r + P (P^T A P)^-1 P^T r (k_coarse.hip) against the oracle's restatement (eo_sim.coarse_m): the coarse matrix is
    assembled from integer sums (exact), factored and inverted on the device, and the coarse sums of r are folded in another order
    than the oracle's row-major loop - so the comparison is to rounding, not to the bit.  (a) iterates: with the budget capped at 5
    iterations the pressures of three consecutive substeps agree to 1e-11 of max |p| (measured 1e-14..2e-13) and the residuals to
    1e-9 relative; (b) solves run to the reference's tolerance: iteration counts within 6 % (rounding differences grow over a
    200-iteration solve: measured 185 vs 194 at worst), pressures within 1e-6 of max |p|, identical cell grids.  Square, flat and
    tall grids."""
    o, sim = _two_level_pair(X, Y, 5)
    for k in range(3):
        dt = sim.timestep(0.1)
        assert dt == o.timestep(0.1)
        sim.substep(dt); o.substep(dt)
        st = sim.stats()
        assert st.last_pcg_iterations == o.c.last_pcg_iterations == 5
        pr = o.p
        assert np.abs(sim.get(ea.F_PRESSURE) - pr).max() <= 1e-11 * np.abs(pr).max(), k
        assert abs(st.last_residual - o.c.last_residual) <= 1e-9 * o.c.last_residual
    sim.close(); o.close()
    o, sim = _two_level_pair(X, Y, 4000)
    for f in range(2):
        o.step(); sim.step()
    st = sim.stats()
    assert st.last_residual <= 1e-6 and o.c.last_residual <= 1e-6
    assert abs(st.total_pcg_iterations - o.c.total_pcg_iterations) <= 0.06 * o.c.total_pcg_iterations + 2, (st.total_pcg_iterations, o.c.total_pcg_iterations)
    p, pr = sim.get(ea.F_PRESSURE), o.p
    assert np.abs(p - pr).max() <= 1e-6 * np.abs(pr).max()
    assert_bits(sim.get(ea.F_COUNT), o.count, "cell grid")
    assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-5 and np.abs(sim.get(ea.F_V) - o.v).max() < 1e-5


def test_two_level_preconditioner_needs_a_fraction_of_the_reference_iterations():
    """512^2 half tank from rest to the reference's tolerance: the reference's IC(0) (parity mode), the tile-local mode and the
    two-level mode reach the same pressure (1e-5 max |p|); the two-level mode in less than half the reference's iterations
    (measured 216 vs 445 vs 594 for the tile-local mode)."""
    res = {}
    for name, pc in (("ic0", ea.PRECOND_IC0), ("tile", ea.PRECOND_IC0_TILE), ("two_level", ea.PRECOND_IC0_TILE2)):
        sim = ea.Simulation(512, 512, dot_mode=ea.DOT_TREE, precond=pc, tile_records=16, max_iterations=5000).load_half_tank()
        sim.step()
        st = sim.stats()
        assert st.last_residual <= 1e-6, name
        res[name] = (st.total_pcg_iterations, sim.get(ea.F_PRESSURE))
        sim.close()
    print({k: v[0] for k, v in res.items()})
    pmax = np.abs(res["ic0"][1]).max()
    assert np.abs(res["two_level"][1] - res["ic0"][1]).max() <= 1e-5 * pmax
    assert res["two_level"][0] < 0.5 * res["ic0"][0]


def test_two_level_mode_moving_water_against_the_oracle():
    """A dam break several bands deep in the two-level mode, solves run to tolerance (budget lifted): free-running against the
    oracle's restatement for 10 frames - cell grids and marker counts identical, velocities within 1e-4 (converged solves differ by
    the tolerance, not by iterates), switching between the modes on a live handle included."""
    text = scenario_text(load("block_frames.npz"))
    o, sim = _two_level_pair(384, 448, 4000, text)
    for f in range(10):
        o.step(); sim.step()
        assert_bits(sim.get(ea.F_COUNT), o.count, "count frame %d" % f)
        assert sim.stats().n_markers == o.n_markers
        assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-4 and np.abs(sim.get(ea.F_V) - o.v).max() < 1e-4, f
    sim.set_precond(ea.PRECOND_IC0)            # and back to the reference's preconditioner on the same handle
    o.c.tile_records = 0; o.c.coarse_m = 0
    o.step(); sim.step()
    assert_bits(sim.get(ea.F_COUNT), o.count, "count after switching back")
    assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-4


def test_two_level_mode_refuses_what_it_cannot_do():
    """single preconditioner operations (the coarse level lives inside a solve), tile widths other than 16"""
    sim = ea.Simulation(260, 300, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE2).load_half_tank()
    sim.pcg_op(ea.OP_BUILD_SYSTEM, dt=0.05)
    with pytest.raises(ea.EulerError):
        sim.pcg_op(ea.OP_BACKWARD_SOLVE)
    with pytest.raises(ea.EulerError):
        sim.set_precond(ea.PRECOND_IC0_TILE2, 8)
    sim.set_precond(ea.PRECOND_IC0_TILE, 8)       # the tile level alone takes any width
    sim.pcg_op(ea.OP_BACKWARD_SOLVE)
    sim.step()
    assert sim.stats().last_residual <= 1e-6 or sim.stats().last_pcg_iterations == 100


# ----------------------------------------------------------------------------- multilevel preconditioner (EULER_PRECOND_IC0_TILE_MG)
@pytest.mark.parametrize("X,Y", [(100, 40), (260, 300), (1100, 200), (130, 1030), (1536, 1280)])
def test_multilevel_preconditioner_matches_the_oracle_restatement(X, Y):
    """z = M_tile^-1 r + P_0 V(P_0^T r) (k_mg.hip, k_mg_cycle.hip) against the oracle's restatement (eo_sim.coarse_mg, mg_build / mg_vcycle): level 0's
    stencil is an integer sum (exact), the coarser ones and the V-cycle use the oracle's formulas with sums folded in another order - agreement to rounding.  (a) budget capped at 5: pressures of the first substep to 1e-11 of max |p| (measured 2e-15..4e-13),
    residuals to 1e-9; (b) to the reference's tolerance: the same iteration counts within 3 % (measured: identical), pressures within 1e-6 of
    max |p|, identical cell grids.  Square, flat, tall; 1536 x 1280 has coarse_m = 2, i.e. three levels below the dense one."""
    o, sim = _two_level_pair(X, Y, 5, mg=True)
    dt = sim.timestep(0.1)
    assert dt == o.timestep(0.1)
    sim.substep(dt); o.substep(dt)
    st = sim.stats()
    assert st.last_pcg_iterations == o.c.last_pcg_iterations == 5
    pr = o.p
    assert np.abs(sim.get(ea.F_PRESSURE) - pr).max() <= 1e-11 * np.abs(pr).max()
    assert abs(st.last_residual - o.c.last_residual) <= 1e-9 * o.c.last_residual
    sim.close(); o.close()
    o, sim = _two_level_pair(X, Y, 4000, mg=True)
    o.step(); sim.step()
    st = sim.stats()
    assert st.last_residual <= 1e-6 and o.c.last_residual <= 1e-6
    assert abs(st.total_pcg_iterations - o.c.total_pcg_iterations) <= 0.03 * o.c.total_pcg_iterations + 2, (st.total_pcg_iterations, o.c.total_pcg_iterations)
    p, pr = sim.get(ea.F_PRESSURE), o.p
    assert np.abs(p - pr).max() <= 1e-6 * np.abs(pr).max()
    assert_bits(sim.get(ea.F_COUNT), o.count, "cell grid")
    assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-5 and np.abs(sim.get(ea.F_V) - o.v).max() < 1e-5


def test_multilevel_mode_4096_half_tank_against_the_recorded_oracle():
    """The oracle's restatement of the multilevel mode at 4096^2 (tests/golden/mg_records.npz, make_mg_records.py: 20 s of one core in the build container; the 8192^2
    record is checked in test_gpu_parity.py::test_full_size_8192_half_tank_properties): the same dt and marker count, the iteration count within 3 %, max |p| and the
    pressure on a 64 x 64 sample grid within 1e-6 max |p|."""
    from test_gpu_parity import mg_record, mg_sample
    sc, ps = mg_record("half_tank_4096_mg")
    N = 4096
    sim = ea.Simulation(N, N, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=4000).load_half_tank()
    dt = sim.timestep(0.1)
    assert dt == np.float32(sc[3])
    sim.substep(dt)
    st = sim.stats()
    assert st.n_markers == int(sc[4]) and st.last_residual <= 1e-6
    assert abs(st.last_pcg_iterations - sc[0]) <= 0.03 * sc[0] + 2, (st.last_pcg_iterations, sc[0])
    p = sim.get(ea.F_PRESSURE)
    assert abs(np.abs(p).max() - sc[2]) <= 1e-6 * sc[2] and np.abs(mg_sample(p) - ps).max() <= 1e-6 * sc[2]
    sim.close()


def test_multilevel_mode_2048_dam_break_against_the_recorded_oracle():
    """configs[1] / [3]'s scenario at 2048^2 in the multilevel mode, free-running from frame 0 against the oracle's restatement recorded in the build container
    (tests/golden/mg_records.npz, make_mg_records.py).  The block falls freely for most of a hundred frames - whatever solves on the way work on rounding noise (max p ~ 1e-4,
    nothing to compare) - and the record holds the six frames from the IMPACT on (max p > 10), every substep solved to the reference's tolerance.  Two tolerance-converged
    runs of a splash are not bit-identical (the GPU folds its sums in another order from the first noise solve on), so per recorded frame: the same substep count, the
    marker count, the number of fluid cells within 1e-4, the iteration count within 5 % (+ 3), max |p| within 2e-5 and the pressure on a 64 x 64 sample grid within
    2e-4 max |p| (measured: identical iteration counts 185 / 395 / 332 / 323 / 323 / 330, identical cell and marker counts, max |p| to 1.6e-6, the samples to 0 ... 1.7e-5:
    the bounds are ten times that)."""
    from euler_amd import scenarios
    from test_gpu_parity import mg_record, mg_sample
    sc, ps = mg_record("dam_break_2048_mg")
    N = 2048
    sim = ea.Simulation(N, N, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=4000).load_text(scenarios.dam_break(), upscale=True)
    k, dev = 0, []
    for frame in range(1, int(sc[-1][0]) + 1):
        sim.step()
        st = sim.stats()
        assert st.last_residual <= 1e-6 and st.last_pcg_iterations <= 60 * st.last_substeps, (frame, st.last_pcg_iterations, st.last_substeps, st.last_residual)
        if frame != int(sc[k][0]):
            continue
        fr, nsub, its, res, pmax, nmark, nfluid, umax, vmax = sc[k]
        p = sim.get(ea.F_PRESSURE)
        nf = int((sim.get(ea.F_COUNT) > 0).sum())
        d = float(np.abs(mg_sample(p) - ps[k]).max() / pmax)
        dev.append((frame, st.last_substeps, int(nsub), st.last_pcg_iterations, int(its), round(float(np.abs(p).max() / pmax - 1.0), 9), round(d, 9), nf - int(nfluid), st.n_markers - int(nmark)))
        k += 1
    print(dev)
    assert k == len(sc)
    for frame, ns, ns_o, it, it_o, dpm, d, dnf, dnm in dev:
        assert ns == ns_o and dnm == 0, dev
        assert abs(it - it_o) <= 0.05 * it_o + 3, dev
        assert abs(dnf) <= 1e-4 * nfluid and abs(dpm) <= 2e-5 and d <= 2e-4, dev
    sim.close()


def test_multilevel_mode_with_spray_above_the_pool_matches_the_oracle():
    """The per-node damping of the cycle's Jacobi steps (k_mg_wd; oracle: mg_damping; tests/test_oracle_tile.py has the story): a pool with 200 single-cell drops above it
    solves in the iterations of a pool without them, on the GPU as in the oracle, and five capped iterations agree to rounding."""
    from test_oracle_tile import _spray_text
    X, Y = 256, 192
    text = _spray_text(X - 5, Y - 2, 200)
    for maxit in (5, 4000):
        o = Oracle(X, Y).load_text(text, upscale=False)
        o.c.tile_records = 16; o.c.coarse_m = o.lib.eo_coarse_m(X, Y); o.c.coarse_mg = 1; o.c.max_iterations = maxit
        sim = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=maxit).load_text(text, upscale=False)
        o.step(); sim.step()
        st = sim.stats()
        pr = o.p
        if maxit == 5:
            assert st.last_pcg_iterations == o.c.last_pcg_iterations == 5
            assert np.abs(sim.get(ea.F_PRESSURE) - pr).max() <= 1e-11 * np.abs(pr).max()
        else:
            assert st.last_residual <= 1e-6 and o.c.last_residual <= 1e-6
            assert abs(st.last_pcg_iterations - o.c.last_pcg_iterations) <= 2 and st.last_pcg_iterations <= 36, (st.last_pcg_iterations, o.c.last_pcg_iterations)
            assert np.abs(sim.get(ea.F_PRESSURE) - pr).max() <= 1e-6 * np.abs(pr).max()
        assert_bits(sim.get(ea.F_COUNT), o.count, "cell grid")
        sim.close(); o.close()


def test_multilevel_iteration_counts_do_not_grow_with_the_grid():
    """Half tank from rest to the reference's tolerance at 512^2, 1024^2, 2048^2: the multilevel mode needs ~30 iterations at every size (bilinear
    coarse spaces on nodes 8 cells apart, round 5; rounds 3-4's piecewise-constant aggregates of 16: 107 / 108 / 118) where the reference's IC(0) needs 445 / 880 / 1726, and
    reaches the reference's pressure (1e-5 of max |p|, checked at 512^2 against the parity mode)."""
    its = {}
    for n in (512, 1024, 2048):
        sim = ea.Simulation(n, n, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=5000).load_half_tank()
        dt = sim.timestep(0.1)
        sim.substep(dt)
        st = sim.stats()
        assert st.last_residual <= 1e-6
        its[n] = st.last_pcg_iterations
        if n == 512:
            ref = ea.Simulation(n, n, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0, max_iterations=5000).load_half_tank()
            ref.substep(dt)
            pr = ref.get(ea.F_PRESSURE)
            assert np.abs(sim.get(ea.F_PRESSURE) - pr).max() <= 1e-5 * np.abs(pr).max()
            its["ic0_512"] = ref.stats().last_pcg_iterations
            ref.close()
        sim.close()
    print(its)
    assert all(24 <= its[n] <= 40 for n in (512, 1024, 2048)), its
    assert its[512] < 0.1 * its["ic0_512"]


def test_multilevel_mode_moving_water_against_the_oracle():
    """A dam break several bands deep, solves run to tolerance: free-running against the oracle's restatement for 10 frames - cell grids and
    marker counts identical, velocities within 1e-4; then back to the reference's preconditioner on the same handle."""
    text = scenario_text(load("block_frames.npz"))
    o, sim = _two_level_pair(384, 448, 4000, text, mg=True)
    for f in range(10):
        o.step(); sim.step()
        assert_bits(sim.get(ea.F_COUNT), o.count, "count frame %d" % f)
        assert sim.stats().n_markers == o.n_markers
        assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-4 and np.abs(sim.get(ea.F_V) - o.v).max() < 1e-4, f
    sim.set_precond(ea.PRECOND_IC0)
    o.c.tile_records = 0; o.c.coarse_m = 0; o.c.coarse_mg = 0
    o.step(); sim.step()
    assert_bits(sim.get(ea.F_COUNT), o.count, "count after switching back")
    assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-4


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("mg", [False, True])
def test_coarse_modes_on_random_scenes(seed, mg):
    """Random walls, pools and air pockets (a 44 x 36 character scene upscaled to 300 x 260: aggregates without fluid, aggregates cut by walls,
    fluid in single cells): two-level and multilevel modes against the oracle's restatements - iterates capped at 5 to 1e-10 of max |p| for
    three substeps of moving water, then a frame solved to tolerance with the same cell grid and iteration counts within 5 %."""
    text = random_scene_text(seed)
    o, sim = _two_level_pair(300, 260, 5, text, mg=mg)
    for k in range(3):
        dt = sim.timestep(0.1)
        assert dt == o.timestep(0.1)
        sim.substep(dt); o.substep(dt)
        st = sim.stats()
        assert st.last_pcg_iterations == o.c.last_pcg_iterations
        pr = o.p
        if k == 0:      # (later substeps inherit float32 velocities that may round apart)
            assert np.abs(sim.get(ea.F_PRESSURE) - pr).max() <= 1e-10 * max(np.abs(pr).max(), 1e-30), k
        assert_bits(sim.get(ea.F_COUNT), o.count, "cell grid, substep %d" % k)
    sim.close(); o.close()
    o, sim = _two_level_pair(300, 260, 4000, text, mg=mg)
    o.step(); sim.step()
    assert sim.stats().last_residual <= 1e-6 and o.c.last_residual <= 1e-6
    assert abs(sim.stats().total_pcg_iterations - o.c.total_pcg_iterations) <= 0.05 * o.c.total_pcg_iterations + 3, (sim.stats().total_pcg_iterations, o.c.total_pcg_iterations)
    assert_bits(sim.get(ea.F_COUNT), o.count, "cell grid")
    assert np.abs(sim.get(ea.F_U) - o.u).max() < 1e-4 and np.abs(sim.get(ea.F_V) - o.v).max() < 1e-4


def _closed_boxes():
    """(a) a closed box completely full of water, (b) the same with a walled-in air pocket: in both the water has no contact with the air
    outside a wall - A is singular along the indicator of that fluid region (pure Neumann)"""
    W, H = 40, 30
    rows = ["X" * W] + ["X" + "0" * (W - 2) + "X" for _ in range(H - 2)] + ["X" * W]
    full = "\n".join(rows) + "\n"
    rows2 = list(rows)
    for y in range(8, 16):
        rows2[y] = rows2[y][:10] + "X" + " " * 8 + "X" + rows2[y][20:]
    rows2[7] = rows2[7][:10] + "X" * 10 + rows2[7][20:]
    rows2[16] = rows2[16][:10] + "X" * 10 + rows2[16][20:]
    return {"closed full box": full, "box with a walled-in air pocket": "\n".join(rows2) + "\n"}


@pytest.mark.parametrize("case", ["closed full box", "box with a walled-in air pocket"])
@pytest.mark.parametrize("mg", [False, True])
def test_coarse_modes_on_fluid_cut_off_from_the_air(case, mg):
    """Water without contact to the air makes A - and the coarse matrix - singular.  The factor pins one coarse cell of such a component (the pivot
    falls back to the diagonal, as main.c:595 does for its own factor) and k_coarse_nullfix takes the component's indicator out of the inverse
    again (pseudo-inverse): every solve converges like with the reference's IC(0) (before the fix: stalls at residuals up to 1e5), to the same
    cell grid, in fewer iterations; and the GPU stays in step with the oracle's restatement."""
    text = _closed_boxes()[case]
    ref = ea.Simulation(320, 256, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0, max_iterations=3000).load_text(text, upscale=True)
    o, sim = _two_level_pair(320, 256, 3000, text, mg=mg)
    for f in range(8):
        ref.step(); sim.step(); o.step()
        st = sim.stats()
        assert st.last_residual <= 1e-6 and ref.stats().last_residual <= 1e-6 and o.c.last_residual <= 1e-6, (f, st.last_residual, o.c.last_residual)
        assert abs(st.last_pcg_iterations - o.c.last_pcg_iterations) <= 0.1 * o.c.last_pcg_iterations + 5, (f, st.last_pcg_iterations, o.c.last_pcg_iterations)
    assert sim.stats().total_pcg_iterations < 0.8 * ref.stats().total_pcg_iterations
    # the same cells hold water as with the reference's IC(0) (the counts inside them are marker positions to 1e-6: they may differ by one), the same flow
    assert np.array_equal(sim.get(ea.F_COUNT) > 0, ref.get(ea.F_COUNT) > 0)
    assert np.abs(sim.get(ea.F_U) - ref.get(ea.F_U)).max() < 1e-3 and np.abs(sim.get(ea.F_V) - ref.get(ea.F_V)).max() < 1e-3


def test_closed_box_right_hand_side_is_made_compatible():
    """b of a closed box (float divergences) is compatible with the singular A only to rounding; before eu_launch_coarse_consistent took the part of b along the
    region's indicator out, one solve in six of this run wandered for 2000 iterations after missing the tolerance narrowly (oracle and GPU alike).  Now: ~100 each,
    in step with the oracle."""
    text = _closed_boxes()["closed full box"]
    o, sim = _two_level_pair(160, 128, 2000, text, mg=True)
    for f in range(8):
        sim.step(); o.step()
        st = sim.stats()
        assert st.last_residual <= 1e-6 and o.c.last_residual <= 1e-6
        assert st.last_pcg_iterations <= 160 and o.c.last_pcg_iterations <= 160, (f, st.last_pcg_iterations, o.c.last_pcg_iterations)
        assert abs(st.last_pcg_iterations - o.c.last_pcg_iterations) <= 12, (f, st.last_pcg_iterations, o.c.last_pcg_iterations)


def test_set_precond_validates_before_it_changes_anything_and_restores_the_dot_mode():
    """a refused euler_set_precond leaves the handle as it was (the tile width used to change before the mode was checked), and a handle created with
    EULER_DOT_SEQUENTIAL - the reference's order of the dot products, the bit-identical parity mode - gets that mode back when it leaves a coarse mode (which
    folds trees): after IC0 -> multilevel -> IC0 the run continues bit for bit with the oracle."""
    sim = ea.Simulation(130, 70, dot_mode=ea.DOT_SEQUENTIAL, precond=ea.PRECOND_IC0_TILE, tile_records=8).load_half_tank()
    o = Oracle(130, 70).load_half_tank()
    o.c.tile_records = 8
    with pytest.raises(ea.EulerError):
        sim.set_precond(ea.PRECOND_IC0_TILE2, 32)          # the coarse modes run on tiles of 16: refused ...
    with pytest.raises(ea.EulerError):
        sim.set_precond(ea.PRECOND_IC0_TILE, 12)
    sim.step(); o.step()                                   # ... and the tiles are still 8 records wide
    compare_all(o, sim, "tile 8 after a refused call")
    sim.set_precond(ea.PRECOND_IC0_TILE_MG, 16)
    with pytest.raises(ea.EulerError):                     # EULER_OPT_SA_RUN 16 / 32: the parity and the plain tile-local mode only (include/euler.h) ...
        sim.set_option(ea.OPT_SA_RUN, 16)
    assert sim.get_option(ea.OPT_SA_RUN) == 8
    sim.set_precond(ea.PRECOND_IC0, 0)                     # back in the parity mode: sequential dots again
    sim.set_option(ea.OPT_SA_RUN, 16)                      # ... where it is taken
    sim.set_option(ea.OPT_SA_RUN, 8)
    o.c.tile_records = 0
    for f in range(2):
        sim.step(); o.step()
        compare_all(o, sim, "parity mode after a detour through the multilevel mode, frame %d" % f)


def test_a_s_formed_again_in_the_r_update_has_the_stored_forms_bits():
    """k_search_apply does not store A s' (one GPU, tree dots; row slabs with compact ghost rows): the r update - k_precond_tile<16, true>, in the tile-local modes
    and as the other modes' r update - forms it again from s' with the same expression (main.c:679-691).  EULER_OPT_TILE_STORE_AS restores the stored form.  Likewise
    p += alpha s is applied eight iterations at a time out of a ring of eight search arrays (the fmadds of main.c:753 in their order); EULER_OPT_P_STEPS = 2 restores the
    two-array form, 4 a ring of four.  THREE HANDLES OF ONE PROCESS with different options (the default; stored A s' with a ring of four; recomputed A s' with the two
    arrays) step side by side through a few frames of four modes (resident solver off, so that the kernels in question run): the same bits in every field and solver
    vector after every frame."""
    from euler_amd import scenarios
    for name, pc, size, scn, frames in (("tile", ea.PRECOND_IC0_TILE, (448, 320), "dam_break", 45), ("mg", ea.PRECOND_IC0_TILE_MG, (384, 320), "dam_break", 45),
                                        ("ic0", ea.PRECOND_IC0, (320, 448), "waterfall", 6), ("jacobi", ea.PRECOND_JACOBI, (257, 193), "waterfall", 6)):
        sims = [ea.Simulation(size[0], size[1], dot_mode=ea.DOT_TREE, precond=pc, resident=ea.RESIDENT_OFF).load_text(getattr(scenarios, scn)(), upscale=True) for _ in range(3)]
        sims[1].set_option(ea.OPT_TILE_STORE_AS, 1).set_option(ea.OPT_P_STEPS, 4)
        sims[2].set_option(ea.OPT_P_STEPS, 2)
        assert [s.get_option(ea.OPT_P_STEPS) for s in sims] == [8, 4, 2]
        its = 0
        for f in range(frames):
            for s in sims:
                s.step()
            its += sims[0].stats().last_pcg_iterations
            for fld in (ea.F_U, ea.F_V, ea.F_PRESSURE, ea.F_PCG_R, ea.F_PCG_Z, ea.F_PCG_S, ea.F_COUNT):
                a = sims[0].get(fld)
                assert_bits(sims[1].get(fld), a, "%s frame %d field %d: stored A s', ring of four" % (name, f, fld))
                assert_bits(sims[2].get(fld), a, "%s frame %d field %d: two search arrays" % (name, f, fld))
        assert its > 50, (name, its)      # the solves iterated
        for s in sims:
            s.close()
    with pytest.raises(ea.EulerError):      # a refused option leaves the handle as it was
        ea.Simulation(64, 64).set_option(ea.OPT_P_STEPS, 3)
