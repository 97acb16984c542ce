"""z formed twice (tile-local mode, one GPU): k_precond_tile leaves only z's halo and the next k_search_apply forms z again from r with the same tile
solve (k_pcg.h tile_solve / tile_z_recompute).  EULER_OPT_TILE_STORE_Z = 1 restores the stored form.  Two handles of one process, one per form, step
side by side: every field and solver vector - z included, which every solve leaves whole - has the same bits after every frame."""
import numpy as np
import pytest

import euler_amd as ea
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

FIELDS = (ea.F_U, ea.F_V, ea.F_PRESSURE, ea.F_COUNT, ea.F_PCG_R, ea.F_PCG_Z, ea.F_PCG_S)


def _pair(X, Y, scene=None, **kw):
    from euler_amd import scenarios
    sims = []
    for store in (0, 1):
        s = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, resident=ea.RESIDENT_OFF, **kw)
        if scene == "half_tank":
            s.load_half_tank()
        elif scene is not None:
            s.load_text(scene if "\n" in scene else getattr(scenarios, scene)(), upscale=True)
        s.set_option(ea.OPT_TILE_STORE_Z, store)
        sims.append(s)
    assert [s.get_option(ea.OPT_TILE_STORE_Z) for s in sims] == [0, 1]
    return sims


def _same(sims, what, fields=FIELDS):
    for fld in fields:
        assert_bits(sims[0].get(fld), sims[1].get(fld), "%s field %d" % (what, fld))
    a, b = sims[0].stats(), sims[1].stats()
    assert (a.total_pcg_iterations, a.last_pcg_iterations, a.total_substeps) == (b.total_pcg_iterations, b.last_pcg_iterations, b.total_substeps), what


def _frames(sims, n, what):
    its = 0
    for f in range(n):
        for s in sims:
            s.step()
        its += sims[0].stats().last_pcg_iterations
        _same(sims, "%s frame %d" % (what, f))
    return its


@pytest.mark.parametrize("X,Y,scene,frames", [
    (449, 321, "dam_break", 30),      # X not a multiple of 16, Y not of 64; the surface moves: tiles turn interior and back
    (300, 50, "dam_break", 20),       # a single band
    (257, 193, "waterfall", 12),      # sparse water
])
def test_z_formed_twice_has_the_stored_forms_bits(X, Y, scene, frames):
    for tol, max_it in ((None, 100), (0.0, 100), (0.0, 3)):      # converged solves (the pass at the end forms z whole), the capped budget, a tiny budget
        sims = _pair(X, Y, scene, max_iterations=max_it, tol=tol)
        its = _frames(sims, frames, "%dx%d %s tol %s max %d" % (X, Y, scene, tol, max_it))
        assert its > 2 * frames
        for s in sims:
            s.close()


def test_z_formed_twice_all_zero_rhs_and_single_operations():
    # b = 0 (a walled box without water): no solve iterates, z is what the handle had
    box = "\n".join("X" * 20 if y in (0, 9) else "X" + " " * 18 + "X" for y in range(10)) + "\n"
    sims = _pair(130, 70, box)
    for s in sims:
        s.step()
    _same(sims, "empty")
    for s in sims:
        s.close()
    # single building blocks and stage calls behind a solve of the new form read the z it left
    sims = _pair(449, 321, "dam_break")
    _frames(sims, 6, "before ops")
    for op in (ea.OP_DOT_ZR, ea.OP_DOT_ZS):
        va, vb = (s.pcg_op(op) for s in sims)
        assert np.float64(va).tobytes() == np.float64(vb).tobytes(), op
    _same(sims, "after dot ops")
    for s in sims:
        s.pcg_op(ea.OP_UPDATE_SEARCH, scalar=0.5)
    _same(sims, "after update_search")
    dts = [s.timestep(0.1) for s in sims]
    assert dts[0] == dts[1]
    for st in (ea.STAGE_ADVECT_MARKERS, ea.STAGE_REFRESH_COUNTS, ea.STAGE_SOURCES, ea.STAGE_EXTRAPOLATE, ea.STAGE_ADVECT_VELOCITY, ea.STAGE_PROJECT):
        for s in sims:
            s.stage(st, dts[0])
    _same(sims, "after euler_stage")
    _frames(sims, 3, "after stages")
    for s in sims:
        s.close()


def test_z_formed_twice_option_and_mode_switches_on_a_live_handle():
    sims = _pair(449, 321, "dam_break")
    _frames(sims, 5, "start")
    sims[0].set_option(ea.OPT_TILE_STORE_Z, 1)      # the stored form for a while, then back
    _frames(sims, 3, "toggled to stored")
    sims[0].set_option(ea.OPT_TILE_STORE_Z, 0)
    _frames(sims, 3, "toggled back")
    for s in sims:
        s.set_precond(ea.PRECOND_IC0)               # the parity mode never runs the form
    _frames(sims, 2, "parity mode")
    for s in sims:
        s.set_precond(ea.PRECOND_IC0_TILE_MG)       # nor the multilevel mode
    _frames(sims, 2, "multilevel mode")
    for s in sims:
        s.set_precond(ea.PRECOND_IC0_TILE, 16)
    _frames(sims, 4, "tile-local mode again")
    for s in sims:
        s.close()


def test_z_formed_twice_8192_half_tank():
    # the headline's configuration: tol = 0, exactly 100 iterations per solve
    sims = _pair(8192, 8192, "half_tank", max_iterations=100, tol=0.0)
    _frames(sims, 2, "8192^2 half tank")
    for s in sims:
        s.close()
