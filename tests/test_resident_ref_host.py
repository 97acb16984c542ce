"""The helpers of the resident solver's capped-iterate tests (resident_ref.py) and the scenes they run on, checked with the oracle alone: b - A p from the
cell-mask encoding is the oracle's own b - eo_apply_a(p), and every scene gives the GPU tests something to see - a right-hand side, exactly k iterations, an
iterate that still moves, a float solve that differs from the double one, walls on every side of some fluid cell, fluid in several bands."""
import numpy as np
import pytest

import resident_ref as rr


@pytest.mark.parametrize("name", rr.RANDOM)
def test_true_residual_agrees_with_the_oracle(name):
    o = rr.oracle_from_state(rr.scene_state(name))
    o.c.max_iterations = 5
    o.c.tol = 0.0
    o.substep(o.timestep(0.1))
    p = np.array(o.p)
    ap = np.zeros_like(p)
    o.lib.eo_apply_a(o.ptr, o.f64p(p), o.f64p(ap))
    fl = o.count != 0
    want = np.where(fl, o.b - ap, 0.0)
    got = rr.true_residual(o.b, p, rr.oracle_cellmask(o))
    assert got.dtype == np.longdouble
    scale = np.abs(o.b).max()
    assert scale > 0 and np.abs(got - want).max() <= 1e-12 * scale
    # the same on a pressure nothing has clamped: the solver's own recurrence r is b - A p of its unclamped p on every cell the clamp has not touched
    keep, _ = rr.unclamped(p, rr.oracle_cellmask(o))
    assert keep.sum() > 10000 and np.abs(got - o.r)[keep].max() <= 1e-12 * scale
    o.close()


@pytest.mark.parametrize("name,k", rr.ITERATE_CASES)
def test_every_scene_runs_exactly_k_iterations_that_still_move_the_pressure(name, k):
    c = rr.scene_capped(name, k)
    assert np.abs(c.b).max() > 0                      # a right-hand side: the solver is entered at all
    assert c.iterations == k                          # no early exit at tol 0
    assert np.isfinite(c.p).all() and np.abs(c.p).max() > 0      # (not everything clamped away)
    before = rr.scene_capped(name, k - 1).p if k > 1 else np.zeros_like(c.p)
    assert np.abs(c.p - before).max() > 0             # iteration k does something
    assert np.array_equal(c.count, rr.scene_capped(name, 1).count)


@pytest.mark.parametrize("name,k", rr.F32_CASES)
def test_the_float_restatement_differs_from_the_double_solve(name, k):
    c, c32 = rr.scene_capped(name, k), rr.scene_capped(name, k, True)
    assert c32.iterations == c.iterations == k
    e32 = np.abs(c32.p - c.p).max() / np.abs(c.p).max()
    assert 0 < e32 < 1e-5, e32                        # float arithmetic's own error: the yardstick of the f32 test is not empty


@pytest.mark.parametrize("name", rr.RANDOM)
def test_random_scenes_have_walls_on_every_side_and_fluid_in_three_bands(name):
    st = rr.scene_state(name)
    c = rr.scene_capped(name, 1)
    fl, solid = c.count != 0, st["solid"] != 0
    assert (fl[:, 1:] & solid[:, :-1]).any() and (fl[:, :-1] & solid[:, 1:]).any()      # a wall to the left / to the right of a fluid cell
    assert (fl[1:, :] & solid[:-1, :]).any() and (fl[:-1, :] & solid[1:, :]).any()      # below / above
    assert len({y // 64 for y in np.nonzero(fl.any(axis=1))[0]}) >= 3
    # cells at a chunk's ends: the first / last row of a 64-row band next to a wall or to air
    rows = np.arange(fl.shape[0])[:, None] % 64
    assert (fl & (rows == 0)).any() and (fl & (rows == 63)).any()
    assert (st["u"] != 0).any() and (st["v"] != 0).any()                              # the water moves


@pytest.mark.parametrize("name,k", rr.RESIDUAL_CASES)
def test_the_cells_the_clamp_leaves_are_enough(name, k):
    c = rr.scene_capped(name, k)
    keep, share = rr.unclamped(c.p, c.cellmask)
    assert keep.any(), (name, k)
    assert np.abs(rr.true_residual(c.b, c.p, c.cellmask) - c.r)[keep].max() <= 1e-12 * np.abs(c.b).max()
    assert abs(np.abs(c.r).max() - c.residual) == 0
    if (name, k) in rr.CLAMP_FIT:
        assert share < rr.CLAMP_CAP, (name, k, share)


def test_clamp_fit_lists_exactly_the_cases_under_the_cap():
    fit = [(n, k) for n, k in rr.RESIDUAL_CASES if rr.unclamped(rr.scene_capped(n, k).p, rr.scene_capped(n, k).cellmask)[1] < rr.CLAMP_CAP]
    assert fit == rr.CLAMP_FIT
