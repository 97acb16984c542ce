"""The resident solver's (csrc/k_resident.hip) CAPPED iterates: after k iterations with tol = 0 nothing has repaired itself yet - a wrong halo address, a halo s'
that differs from the owner's, a stale halo cell or a preconditioner off in one lane sits in p and r at full size.  Scenes with walls, pools, air pockets, ragged
grids and grids of a single chunk (resident_ref.py; the oracle-only half is test_resident_ref_host.py), every handle teacher-forced from one oracle state.

Handle `a` is resident, `b` the same with RESIDENT_OFF (the multi-kernel tile mode, also tree sums), the oracle runs tile_records = 16 with sequential sums."""
import numpy as np
import pytest

import euler_amd as ea
import resident_ref as rr

pytestmark = pytest.mark.gpu

FIELDS = ((ea.F_SOLID, "solid"), (ea.F_SOURCE, "source"), (ea.F_SINK, "sink"), (ea.F_COUNT, "count"), (ea.F_PREV_COUNT, "prev_count"),
          (ea.F_U, "u"), (ea.F_V, "v"), (ea.F_UTMP, "utmp"), (ea.F_VTMP, "vtmp"), (ea.F_PRECON, "precon"))


def load_state(sim, state):
    for f, n in FIELDS:
        sim.set(f, state[n])
    sim.set_markers(state["markers"])
    sim.set_rng(state["rng_state"], state["source_exhausted"])
    return sim


def handle(state, k, **kw):
    return load_state(ea.Simulation(state["X"], state["Y"], dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, tile_records=16, tol=0.0, max_iterations=k, **kw), state)


def substep(sim):
    dt = sim.timestep(0.1)
    sim.substep(dt)
    return dt


def ran_resident(sim):
    info = sim.resident_info()
    assert info[0] and info[1] >= 1 and info[2] == 0, info      # eligible, the solve ran resident, nothing fell back: no other path can have made the result


def distance(p, ref):
    return float(np.abs(p - ref).max() / np.abs(ref).max())


def capped_against_the_oracle(state, k, ref, a):
    """dt, iteration count, cell grid and the pressure bound of the f64 iterates: `a` (already created, state loaded) and a RESIDENT_OFF handle against `ref`"""
    b = handle(state, k, resident=ea.RESIDENT_OFF)
    assert substep(a) == substep(b) == ref.dt
    assert a.stats().last_pcg_iterations == b.stats().last_pcg_iterations == ref.iterations == k
    assert np.array_equal(a.get(ea.F_COUNT), ref.count) and np.array_equal(b.get(ea.F_COUNT), ref.count)
    d_mk, d_res = distance(b.get(ea.F_PRESSURE), ref.p), distance(a.get(ea.F_PRESSURE), ref.p)
    b.close()
    return d_mk, d_res


@pytest.mark.parametrize("name,k", rr.ITERATE_CASES)
def test_capped_f64_iterates_against_the_oracle(name, k):
    """One substep capped at k = 1 (no tile solve, no publish: the budget's last iteration; the halo of z_0), 2 (the first beta and the halo's s), 3, 5, 17.
    D_mk = max |p_b - p_oracle| / max |p_oracle| is what a second summation order (the multi-kernel path's trees against the oracle's sequential sums) costs, measured
    live; the resident pressure must stay within max(10 D_mk, 1e-11) - ten times for two tree shapes against one sequential order, 1e-11 the bar of the coarse modes'
    capped iterates.  A halo cell from the wrong address moves p by O(1) of max |p| from k = 2 on.
    Measured on an MI355X, worst over the scenes, D_mk / resident: k = 1: 8.2e-15 / 8.5e-15, 2: 9.0e-15 / 9.0e-15, 3: 7.6e-15 / 7.4e-15, 5: 1.6e-14 / 1.6e-14,
    17: 8.9e-15 / 8.5e-15 - D_mk stays a thousand times under 1e-11 / 10, so the floor is the bound that acts."""
    state, ref = rr.scene_state(name), rr.scene_capped(name, k)
    a = handle(state, k)
    d_mk, d_res = capped_against_the_oracle(state, k, ref, a)
    print("capped f64 %s k=%d: D_mk %.3g resident %.3g" % (name, k, d_mk, d_res))
    ran_resident(a)
    assert d_res <= max(10 * d_mk, 1e-11), (d_res, d_mk)
    a.close()


@pytest.mark.parametrize("name,k", rr.RESIDUAL_CASES)
def test_the_residual_the_resident_solver_reports_is_the_true_residual(name, k):
    """r of a resident solve is a recurrence in registers; here it is held to b - A p (long double, A from the cell mask) to 1e-9 max |b| - the bound of
    test_reported_residual_is_the_true_residual_2048 - and stats().last_residual to max |r|.  The pressure a caller reads is clamped (p < 0 -> 0) and a capped
    iterate of moving water is negative over much of the fluid, so the comparison runs on the cells whose row of A p holds no clamped cell (resident_ref.unclamped);
    the share left out is printed, and asserted under 5 % where the oracle alone meets that (resident_ref.CLAMP_FIT: weird-edges, the dam break from k = 5 on;
    random scenes leave out 44 - 55 % and keep 17 000 - 21 000 cells, the dam break 6.9 % at k = 1, the stirred one-band grids 83 - 94 %).
    Measured on an MI355X: max |true r - r| / max |b| = 1e-16 ... 1.0e-14 over all cases, shares left out as the oracle's."""
    state = rr.scene_state(name)
    a = handle(state, k)
    substep(a)
    ran_resident(a)
    b, p, r, m = a.get(ea.F_PCG_B), a.get(ea.F_PRESSURE), a.get(ea.F_PCG_R), a.get(ea.F_CELLMASK)
    assert a.stats().last_pcg_iterations == k and np.array_equal((m & 1) != 0, rr.scene_capped(name, k).count != 0)
    keep, share = rr.unclamped(p, m)
    scale = np.abs(b).max()
    err = float(np.abs(rr.true_residual(b, p, m) - r)[keep].max())
    print("residual %s k=%d: left out %.4f of the fluid cells, kept %d, max |true r - r| / max |b| %.3g" % (name, k, share, int(keep.sum()), err / scale))
    assert keep.any()
    assert err <= 1e-9 * scale
    # max |r| over ALL fluid cells is the reported residual; with r = b - A p on the kept cells that ties last_residual to the true residual
    assert abs(np.abs(r).max() - a.stats().last_residual) <= 1e-9 * scale
    assert abs(float(np.abs(rr.true_residual(b, p, m))[keep].max()) - np.abs(r[keep]).max()) <= 1e-9 * scale
    if (name, k) in rr.CLAMP_FIT:
        assert share < rr.CLAMP_CAP, share
    a.close()


@pytest.mark.parametrize("name,k", rr.F32_CASES)
def test_f32_early_iterates_against_the_oracle_float_restatement(name, k):
    """PCG_F32 against eo_sim.pcg_f32 (every operation rounded to float, sums and scalars in double - as in the kernel).  The yardstick E32(k) = max |p_oracle_f32 -
    p_oracle_f64| / max |p_oracle_f64| is float arithmetic's own error, from the reference alone: the kernel must sit nearer to its restatement than float rounding
    sits to double.  Measured on an MI355X: distance 0 - the same bits - in all 25 cases, against E32 = 8.5e-8 ... 7.1e-7."""
    state, ref, ref32 = rr.scene_state(name), rr.scene_capped(name, k), rr.scene_capped(name, k, True)
    e32 = distance(ref32.p, ref.p)
    a = handle(state, k, pcg_precision=ea.PCG_F32)
    assert substep(a) == ref32.dt
    ran_resident(a)
    p = a.get(ea.F_PRESSURE)
    d = float(np.abs(p - ref32.p).max() / np.abs(ref.p).max())
    print("capped f32 %s k=%d: distance %.3g, E32 %.3g" % (name, k, d, e32))
    assert a.stats().last_pcg_iterations == ref32.iterations == k
    assert np.array_equal(a.get(ea.F_COUNT), ref32.count)
    assert np.array_equal(p, p.astype(np.float32).astype(np.float64))      # p holds float values
    assert d <= e32, (d, e32)
    a.close()


def test_nothing_leaks_from_an_earlier_solve():
    """The granules are never cleared and the halo arrays keep what the last solve published.  Handle `a` runs random scene 1 for three frames to tolerance, is then
    overwritten whole with the moving state of scene 2 (another chunk list altogether) and takes one substep capped at 5; a fresh handle takes the same substep.
    The same kernel and fold order: p, r and E^-1 are bit-equal unless a stale halo cell or granule was picked up."""
    X, Y, text = rr.SCENES["random1"][:3]
    a = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, tile_records=16, max_iterations=2000).load_text(text, upscale=True)
    for _ in range(3):
        a.step()
        assert a.stats().last_residual <= 1e-6
    solved = a.resident_info()[1]
    assert solved >= 3 and a.resident_info()[2] == 0
    state = rr.scene_state("random2")
    load_state(a, state)
    a.set_solver(5, 0.0)
    c = handle(state, 5)
    assert substep(a) == substep(c)
    assert a.stats().last_pcg_iterations == c.stats().last_pcg_iterations == 5
    assert a.resident_info() == (True, solved + 1, 0)
    ran_resident(c)
    for f in (ea.F_PRESSURE, ea.F_PCG_R, ea.F_PRECON, ea.F_COUNT):
        assert np.array_equal(a.get(f).view(np.uint8), c.get(f).view(np.uint8)), f
    assert np.abs(a.get(ea.F_PRESSURE)).max() > 0
    a.close(); c.close()


def test_three_fresh_handles_leave_the_same_bits():
    """"the same bits everywhere" (docs/solver_resident.md): a halo read that races its publish, or a fold whose order depends on arrival, shows between runs"""
    state = rr.scene_state("random3")
    got = []
    for _ in range(3):
        a = handle(state, 17)
        substep(a)
        ran_resident(a)
        got.append((a.get(ea.F_PRESSURE), a.get(ea.F_PCG_R)))
        a.close()
    for p, r in got[1:]:
        assert np.array_equal(p.view(np.uint8), got[0][0].view(np.uint8)) and np.array_equal(r.view(np.uint8), got[0][1].view(np.uint8))
    assert np.abs(got[0][0]).max() > 0


def _native_random1():
    X, Y = 46, 38      # the 44 x 36 picture cell for cell: one band, a handful of chunks
    return rr.moving_state(X, Y, rr.random_scene_text(1), 3, upscale=False)


@pytest.mark.parametrize("scene", ["random1", "random1_native_46x38"])
def test_the_capacity_boundary(scene):
    """EULER_OPT_RESIDENT_CAP = 1 .. 8 workgroups, k = 5: whichever path ran, the pressure obeys the bound of the capped-iterate test; "does not fit" is never a
    time-out; and whether the solve ran resident is monotone in the capacity.  At 300 x 260 random scene 1 has over a hundred active chunks - more than eight
    workgroups hold, so every capacity sends it down the multi-kernel path; the same picture on its native 46 x 38 grid has few enough that the boundary lies
    inside the range: it must be seen from both sides there."""
    state = rr.scene_state("random1") if scene == "random1" else _native_random1()
    ref = rr.scene_capped("random1", 5) if scene == "random1" else rr.oracle_capped(state, 5)
    assert ref.iterations == 5 and np.abs(ref.p).max() > 0
    resident = []
    for c in range(1, 9):
        a = ea.Simulation(state["X"], state["Y"], dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, tile_records=16, tol=0.0, max_iterations=5)
        a.set_option(ea.OPT_RESIDENT_CAP, c)
        load_state(a, state)
        d_mk, d_res = capped_against_the_oracle(state, 5, ref, a)
        info = a.resident_info()
        print("capacity %s c=%d: resident solves %d, D_mk %.3g, distance %.3g" % (scene, c, info[1], d_mk, d_res))
        assert d_res <= max(10 * d_mk, 1e-11), (c, d_res, d_mk)
        assert info[2] == 0, (c, info)
        resident.append(info[1] > 0)
        a.close()
    assert resident == sorted(resident), resident      # not resident below some c*, resident from c* on
    if scene != "random1":
        assert resident[0] is False and resident[-1] is True, resident
