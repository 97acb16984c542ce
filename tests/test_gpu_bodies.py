"""euler_set_bodies on the GPU (docs/bodies.md): solid boxes that push water, against the test-side restatement (tests/bodies_ref.py, pinned on the CPU by
test_bodies_host.py), bit for bit in the parity mode (every grid here has fewer than 65 536 cells): the marker stage and the projection teacher-forced, shifts of
one and two cells in every direction, bodies side by side and on top of each other, the clamps, markers on the strips' edges, a strip over source cells, every
alignment of a strip, free runs (each transport, a forcing, the temperature on), the properties (no bodies: no trace; a body at rest: a wall; the lean forms), the piston's known answer in the tile-local and
the multilevel mode, the refusals, the edit next to a body, the loads, and `euler --body`.
The positions of the restatement are euler_body_at's own, so no libm difference reaches these tests."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import bodies_ref as bref
import edit_ref as eref
import euler_amd as ea
import forcing_ref as fref
import heat_ref as href
from euler_amd import scenarios
from observer_util import EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames, no_trace_pair
from oracle_lib import Oracle
from test_bodies_host import CH_X1, CH_Y0, CH_Y1, PISTON_CAP, PISTON_GRID, PISTON_W, PISTON_X, channel_text, lib_at, piston, piston_sections, record
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

GRIDS = [(96, 64), (101, 45), (260, 200)]      # one tile row and a seam at 63 | 64; ragged (one cell per lane); 5 x 4 tiles
F32 = np.float32
MASKS = ((ea.F_SOLID, "solid"), (ea.F_SOURCE, "source"), (ea.F_SINK, "sink"), (ea.F_COUNT, "count"), (ea.F_PREV_COUNT, "prev_count"))


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("bodies_gpu"))


def pair(size, text=None, upscale=True, **kw):
    text = text or scenarios.dam_break()
    sim = ea.Simulation(*size, **kw).load_text(text, upscale=upscale)
    o = Oracle(*size).load_text(text, upscale=upscale)
    return sim, o


def set_both(sim, o, old, old_origins, bodies, t=0.0):
    sim.time = t
    sim.set_bodies([record(b) for b in bodies])
    origins = bref.set_bodies(o, old, old_origins, bodies, t, at=lib_at)
    got, now = sim.bodies()
    assert len(got) == len(bodies) and [[int(s["ox"]), int(s["oy"])] for s in now] == origins
    return origins


def compare_masks(sim, o, what):
    for fld, n in MASKS:
        assert_bits(sim.get(fld), getattr(o, n), "%s %s" % (what, n))
    assert_bits(sim.get(ea.F_MARKERS), o.markers, what + " markers")


def compare_flow(sim, o, what):
    wet = np.array(o.count) != 0
    assert_bits(sim.get(ea.F_U), o.u, what + " u")
    assert_bits(sim.get(ea.F_V), o.v, what + " v")
    assert_bits(np.where(wet, sim.get(ea.F_PRESSURE), 0.0), np.where(wet, np.array(o.p), 0.0), what + " pressure")
    assert_bits(sim.get(ea.F_UTMP), o.utmp, what + " utmp")
    assert_bits(sim.get(ea.F_VTMP), o.vtmp, what + " vtmp")


def origins_of(sim):
    return [[int(s["ox"]), int(s["oy"])] for s in sim.bodies()[1]]


def middle_stages(am, sim, o, dt):
    """the stages between the marker advection and the projection on both sides"""
    lib = o.lib
    sim.stage(ea.STAGE_REFRESH_COUNTS)
    lib.eo_refresh_marker_counts(o.ptr)
    sim.stage(ea.STAGE_SOURCES)
    lib.eo_update_fluid_sources(o.ptr)
    sim.stage(ea.STAGE_EXTRAPOLATE)
    for q, t in ((o.u, 1), (o.v, 2)):
        lib.eo_extrapolate(o.ptr, o.f32p(q), t)
    for q, t in ((o.u, 1), (o.v, 2)):
        lib.eo_zero_bounds(o.ptr, o.f32p(q), t)
    sim.stage(ea.STAGE_ADVECT_VELOCITY, dt)
    fref.advect_velocity_stage(am, o, dt, fref.DEFAULT, (), 0.0)


def forced_substep(am, sim, o, bodies, origins, t_end, what, dt_cap=0.05):
    """One substep stage by stage that ENDS at clock t_end on both sides, compared behind the marker stage and behind the projection; the clock stands still.
    -> the number of unit shifts (the step is left in forced_substep.dt)"""
    dt = sim.timestep(dt_cap)
    assert dt == o.timestep(dt_cap) and 0 < dt <= float(F32(dt_cap))
    t = t_end - float(np.float64(F32(dt)))
    sim.time = t
    X, Y = o.X, o.Y
    tgt = bref.targets(bodies, t, dt, X, Y, at=lib_at)
    shifts = bref.begin_arrays(o.markers, o.solid, o.source, o.sink, o.count, bodies, origins, tgt)
    o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
    sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
    assert sim.time == t and origins_of(sim) == origins == [[g[0], g[1]] for g in tgt]
    compare_masks(sim, o, what + " behind the marker stage")
    middle_stages(am, sim, o, dt)
    compare_masks(sim, o, what + " in front of the projection")
    assert_bits(sim.get(ea.F_UTMP), o.utmp, what + " utmp in front of the projection")
    it = bref.project_stage(o, dt, bodies, origins, tgt)
    sim.stage(ea.STAGE_PROJECT, dt)
    assert sim.stats().last_pcg_iterations == it, (what, sim.stats().last_pcg_iterations, it)
    compare_flow(sim, o, what + " behind the projection")
    lu, lv = fref.live_faces(o.solid, o.count)
    assert not o.utmp[~lu].any() and not o.vtmp[~lv].any()      # the wall velocity is gone again: utmp / vtmp are zero off the live faces
    for b, og in zip(bodies, origins):      # and u = v = 0 on the body's faces
        x0, y0, x1, y1 = bref.rect(b, og)
        assert not o.u[y0:y1 + 1, x0 - 1:x1 + 1].any() and not o.v[y0 - 1:y1 + 1, x0:x1 + 1].any()
    forced_substep.dt = dt
    return shifts


# ----------------------------------------------------------------------------- the two stages, teacher-forced
def scene_bodies(X, Y):
    """Bodies placed relative to the upscaled dam break's block (columns 3 X / 96 .. 53 X / 96, rows 14 Y / 64 .. 48 Y / 64), set at t = 0 and compared at
    t = 0.2: a speed of 8 is a shift of two cells (1.6 rounds to 2), a speed of 4 one cell (0.8 rounds to 1); every direction, and both diagonals."""
    sx, sy = X / 96.0, Y / 64.0
    at = lambda x, y: (int(x * sx), int(y * sy))
    bodies = [bref.body((1, 1), at(20, 25), (8, 0)),            # 1 x 1, two cells to the right
              bref.body((1, 9), at(30, 18), (-4, 0)),           # 1 x 9, one cell to the left
              bref.body((12, 3), at(34, 30), (0, 8)),           # 12 x 3, two cells up
              bref.body((8, 4), (60, int(22 * sy)), (0, -4)),   # across the seam 63 | 64, one cell down
              bref.body((2, 2), at(10, 36), (4, -8)),           # diagonal: one right, two down
              bref.body((3, 3), at(45, 20), (-8, 4)),           # diagonal: two left, one up
              bref.body((2, 5), at(25, 40), (-8, 0)),           # two cells to the left
              bref.body((5, 2), at(15, 20), (0, -8))]           # two cells down
    if X > 140:
        bodies.append(bref.body((6, 70), (125, 40), (4, 0)))    # across 127 | 128 and the seam between the tile rows, one cell to the right
    return bodies


@pytest.mark.parametrize("frame", [0, 6])
@pytest.mark.parametrize("size", GRIDS)
def test_stages_teacher_forced(am, size, frame):
    sim, o = pair(size)
    for _ in range(frame):
        sim.step(); o.step()
    bodies = scene_bodies(*size)
    origins = set_both(sim, o, [], [], bodies)
    what = "%dx%d frame %d" % (size + (frame,))
    compare_masks(sim, o, what + " behind euler_set_bodies")
    shifts = forced_substep(am, sim, o, bodies, origins, 0.2, what)
    assert shifts == 2 + 1 + 2 + 1 + 3 + 3 + 2 + 2 + (1 if size[0] > 140 else 0)
    # a repeated stage call shifts nothing twice: the origins stand, and the marker stage is the plain one
    before = origins_of(sim)
    dt = forced_substep.dt
    sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
    o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
    assert origins_of(sim) == before
    compare_masks(sim, o, what + " behind a repeated marker stage")
    sim.close(); o.close()


# ----------------------------------------------------------------------------- bodies side by side and on top of each other, the clamps
def _pairs_of_bodies():
    a = bref.body((4, 6), (20, 20), (4, 0))
    adjacent = bref.body((3, 6), (24, 20), (4, 0))      # its left face is a's right face
    over = bref.body((5, 5), (22, 23), (0, 8))          # overlaps a
    return {"adjacent": [a, adjacent], "adjacent reversed": [adjacent, a], "overlapping": [a, over], "overlapping reversed": [over, a]}


@pytest.mark.parametrize("case", sorted(_pairs_of_bodies()))
def test_two_bodies_in_both_list_orders(am, case):
    sim, o = pair((96, 64))
    for _ in range(3):
        sim.step(); o.step()
    bodies = _pairs_of_bodies()[case]
    origins = set_both(sim, o, [], [], bodies)
    compare_masks(sim, o, case + " set")
    assert forced_substep(am, sim, o, bodies, origins, 0.2, case) >= 2
    assert forced_substep(am, sim, o, bodies, origins, 0.45, case + " again") >= 2
    sim.close(); o.close()


@pytest.mark.parametrize("size", [(96, 64), (101, 45)])
def test_a_body_held_at_each_clamp(am, size):
    X, Y = size
    sim, o = pair(size)
    bodies = [bref.body((3, 4), (3, 10), (-8, 0)), bref.body((3, 4), (X - 6, 20), (8, 0)),
              bref.body((4, 3), (30, 3), (0, -8)), bref.body((4, 3), (50, Y - 6), (0, 8))]
    origins = set_both(sim, o, [], [], bodies)
    assert forced_substep(am, sim, o, bodies, origins, 0.2, "towards the clamps") == 4 * 1      # each is one cell from its clamp
    assert origins == [[2, 10], [X - 5, 20], [30, 2], [50, Y - 5]]
    assert forced_substep(am, sim, o, bodies, origins, 3.0, "at the clamps") == 0                # held: nothing shifts, no wall velocity
    tgt = bref.targets(bodies, 2.9, 0.05, X, Y, at=lib_at)
    assert all(g[2] == 0 and g[3] == 0 for g in tgt)
    sim.close(); o.close()


# ----------------------------------------------------------------------------- markers on the strips' edges
def test_markers_on_and_below_the_edges_of_a_strip():
    """water at rest (the dam break's frame 0: u = v = 0, the marker advection moves nothing), planted markers: exactly on and one ulp below the four edges of
    each strip, and in column 63 pushed across 64, where the ulp doubles"""
    size = (96, 64)
    sim, o = pair(size)
    bodies = [bref.body((4, 6), (59, 20), (4, 0)),        # strip: column 63, rows 20 .. 25, pushed to column 64
              bref.body((4, 6), (30, 30), (-4, 0)),       # strip: column 29
              bref.body((5, 3), (40, 40), (0, 4)),        # strip: row 43
              bref.body((5, 3), (70, 12), (0, -4))]       # strip: row 11
    origins = set_both(sim, o, [], [], bodies)
    strips = [bref.strips(og[0], og[1], b["w"], b["h"], axis, d)[0] for b, og, (axis, d) in zip(bodies, origins, ((0, 1), (0, -1), (1, 1), (1, -1)))]
    assert strips[0] == (63, 20, 63, 25)
    planted = np.concatenate([eref.edge_markers(s)[0] for s in strips] +
                             [np.array([(np.nextafter(F32(64), F32(0)), 22.5), (63.0, 20.0), (np.nextafter(F32(64), F32(0)), np.nextafter(F32(26), F32(0)))], F32)])
    m = np.concatenate([planted[:7], np.array(o.markers), planted[7:]])      # an odd and an even position for them, the tail of the array included
    sim.set_markers(m); o.set_markers(m)
    dt = float(F32(0.05))
    sim.time = 0.15
    tgt = bref.targets(bodies, 0.15, dt, *size, at=lib_at)
    before = np.array(o.markers)
    assert bref.begin_arrays(o.markers, o.solid, o.source, o.sink, o.count, bodies, origins, tgt) == 4
    pushed = np.array(o.markers)
    o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
    sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
    compare_masks(sim, o, "edge markers")
    assert_bits(np.array(o.markers), pushed, "water at rest: the advection moves nothing")
    moved = (pushed.view(np.uint32) != before.view(np.uint32)).any(axis=1)
    k = len(before) - 3      # the three of column 63: all in the strip, all pushed by fl(x + 1)
    assert moved[k:].all() and pushed[k, 0] == F32(np.nextafter(F32(64), F32(0)) + F32(1)) and pushed[k + 1, 0] == 64.0
    assert np.floor(pushed[k, 0]) in (64.0, 65.0)      # one ulp below the far edge may round into the cell beyond
    # of the eight edge markers of a strip exactly those inside it moved (edit_ref.edge_markers says which)
    idx = list(range(7)) + list(range(7 + len(before) - len(planted), len(before)))
    inside = np.concatenate([eref.edge_markers(s)[1] for s in strips] + [np.array([True, True, True])])
    assert np.array_equal(moved[idx], inside)
    sim.close(); o.close()


# ----------------------------------------------------------------------------- a strip over source cells, every alignment of a strip
def test_a_strip_over_source_cells(am):
    size = (96, 64)
    sim, o = pair(size, scenarios.waterfall())
    src = np.argwhere(np.array(o.source) != 0)
    assert len(src)
    y, x = (int(t) for t in src[len(src) // 2])
    assert 4 <= x <= size[0] - 8 and 3 <= y <= size[1] - 4
    bodies = [bref.body((2, 3), (x - 3, y - 1), (4, 0))]      # its second shift covers the source cell, a later one uncovers it again (carved: no source any more)
    origins = set_both(sim, o, [], [], bodies)
    clock = fref.Clock()
    n_src = [int(np.count_nonzero(o.source))]
    for k in range(12):
        sim.step()
        n, it = bref.step(am, o, bodies, origins, clock, at=lib_at)
        st = sim.stats()
        what = "waterfall frame %d" % k
        assert (st.last_substeps, st.last_pcg_iterations, st.rng_state, st.source_exhausted) == (n, it, int(o.c.rng_state), int(o.c.source_exhausted)), what
        compare_masks(sim, o, what)
        assert origins_of(sim) == origins and sim.time == clock.t
        n_src.append(int(np.count_nonzero(o.source)))
    assert n_src[-1] < n_src[0] and origins[0][0] >= x      # the body has passed over source cells
    sim.close(); o.close()


def test_every_alignment_of_a_strip():
    """X % 4 == 0: the 16 (x0 & 3, x1 & 3) of a horizontal strip (a body that moves up), edge bytes left alone"""
    size = (96, 64)
    sim, o = pair(size)
    old, old_origins = [], []
    dt = float(F32(0.05))
    for r0 in range(4):
        for r1 in range(4):
            x0 = 8 + 4 * (r0 + r1) + r0
            w = 4 * (1 + (r0 * r1) % 3) + r1 - r0 + 1
            assert x0 & 3 == r0 and (x0 + w - 1) & 3 == r1 and w >= 1
            bodies = [bref.body((w, 2), (x0, 16 + 2 * r0), (0, 4))]
            origins = set_both(sim, o, old, old_origins, bodies)
            sim.time = 0.15
            tgt = bref.targets(bodies, 0.15, dt, *size, at=lib_at)
            assert bref.begin_arrays(o.markers, o.solid, o.source, o.sink, o.count, bodies, origins, tgt) == 1
            o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
            sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
            compare_masks(sim, o, "alignment %d %d" % (r0, r1))
            old, old_origins = bodies, origins
    sim.close(); o.close()


# ----------------------------------------------------------------------------- free runs
PISTON_RUN = [bref.body((3, 30), (6, 2), (6, 0))]                                      # a piston through the dam break's block
PADDLE_RUN = [bref.body((2, 24), (30, 2), (0, 0), (5, 0), 0.3), bref.body((6, 2), (60, 30), (0, 0), (0, 1.5), 1.0, 0.7)]      # a paddle and a plunger


def _free_run(am, size, bodies, frames=20, rk2=0, mc=0, f=None, boxes=(), text=None, heat=None):
    """heat = (record, boxes): the temperature on, a striped field in the water, compared after every frame as well"""
    sim, o = pair(size, text)
    sim.set_option(ea.OPT_ADVECT_RK2, rk2)
    sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
    acc_at = None
    if f is not None:
        sim.set_forcing((f["gx"], f["gy"]), (f["shake_x"], f["shake_y"], f["shake_hz"], f["shake_phase"]), boxes)
        acc_at = lambda ff, t: ea.forcing_at(ea.forcing_record((ff["gx"], ff["gy"]), (ff["shake_x"], ff["shake_y"], ff["shake_hz"], ff["shake_phase"])), t)
    T = None
    if heat is not None:
        h, hboxes = heat
        sim.set_heat(h["ambient"], h["beta"], h["kappa"], h["source_t"], list(hboxes))
        ys, xs = np.indices((size[1], size[0]))
        T = (F32(h["ambient"]) + ((xs * 3 + ys * 5) % 9).astype(F32) * F32(0.75) - F32(2.25)).astype(F32)      # something to move in every fluid cell
        T[np.array(o.count) == 0] = F32(h["ambient"])
        sim.temperature = T
    origins = set_both(sim, o, [], [], bodies)
    if heat is not None:      # the cells the new rectangles emptied hold ambient at once, as behind any SOLID edit
        T[np.array(o.count) == 0] = F32(h["ambient"])
        assert_bits(sim.temperature, T, "T behind euler_set_bodies")
    start = [list(og) for og in origins]
    clock = fref.Clock()
    for k in range(frames):
        sim.step()
        n, it = bref.step(am, o, bodies, origins, clock, f, boxes, rk2, mc, acc_at, at=lib_at, heat=None if heat is None else (T, h, hboxes))
        st = sim.stats()
        what = "%dx%d frame %d" % (size + (k,))
        assert (st.last_substeps, st.last_pcg_iterations, st.rng_state) == (n, it, int(o.c.rng_state)), what
        compare_masks(sim, o, what)
        assert_bits(sim.get(ea.F_U), o.u, what + " u")
        assert_bits(sim.get(ea.F_V), o.v, what + " v")
        assert sim.time == clock.t and origins_of(sim) == origins, what
        if heat is not None:
            assert_bits(sim.temperature, T, what + " T")
    assert origins != start and np.abs(o.u).max() > 1
    if heat is not None:
        assert len(np.unique(T)) > 50
    sim.close(); o.close()


@pytest.mark.parametrize("size", GRIDS)
def test_free_run_of_a_piston(am, size):
    _free_run(am, size, PISTON_RUN)


def test_free_run_of_a_paddle_and_a_plunger(am):
    _free_run(am, (96, 64), PADDLE_RUN)


def test_free_run_with_maccormack_and_rk2(am):
    _free_run(am, (96, 64), PISTON_RUN + PADDLE_RUN[1:], rk2=1, mc=1)


def test_free_run_with_a_forcing(am):
    _free_run(am, (101, 45), PISTON_RUN, f=fref.forcing((3.0, -8.0), (1.5, 0.5, 0.8, 0.3)), boxes=[((10, 3, 30, 12), (4.0, -1.5))])


def test_free_run_with_heat_on(am):
    """buoyancy, diffusion, a heater in the piston's way and one in the paddle's: counts, markers in order, RNG, clock and the temperature after every frame"""
    hboxes = [(href.RATE, 30.0, (10, 3, 40, 12)), (href.FIX, 4.0, (25, 8, 45, 30))]
    _free_run(am, (96, 64), PISTON_RUN + PADDLE_RUN[:1], heat=(href.heat(1.0, 0.5, 0.3), hboxes))


def test_dry_cells_hold_ambient_right_after_a_shift():
    sim = ea.Simulation(96, 64).load_text(scenarios.dam_break(), upscale=True)
    sim.set_heat(ambient=2.0, beta=0.0, kappa=0.1)
    sim.heat_fill((1, 1, 94, 62), 5.0)
    sim.set_bodies([record(PISTON_RUN[0])])
    shifted = 0
    for _ in range(6):
        before = origins_of(sim)
        dt = sim.timestep(0.1)
        sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
        shifted += origins_of(sim) != before
        T, count = sim.temperature, sim.get(ea.F_COUNT)
        assert (T[count == 0] == F32(2.0)).all() and (T[count != 0] != F32(2.0)).any()
        for st in range(1, 6):
            sim.stage(st, dt)
        sim.time = sim.time + float(np.float64(F32(dt)))
    assert shifted >= 2
    sim.close()


# ----------------------------------------------------------------------------- the properties
SETTLE_EXTRA = {"marker_bin": 1}      # profile class -> launches a handle runs more than an untouched one in the first frame behind a set and a clear of bodies in the air


def test_no_bodies_leave_no_trace():
    """a handle with n = 0, and one that set and removed bodies away from the water, give an untouched handle's bits and launch counts per profile class"""
    def make():
        s = ea.Simulation(260, 200).load_text(scenarios.dam_break(), upscale=True)
        s.profile_enable(ea.profile_class_names())
        return s

    def look(s, stepped):
        s.clear_bodies()
        assert len(s.bodies()[0]) == 0

    a, b = no_trace_pair(make, look, None, STATE_FIELDS, 12, compare_every=4)
    pa, pb = a.profile(), b.profile()
    assert {k: v[1] for k, v in pa.items()} == {k: v[1] for k, v in pb.items()}
    a.close(); b.close()
    # set and removed in the air, before the first frame: the same masks, the same run
    a, b = make(), make()
    b.set_bodies([record(bref.body((5, 4), (200, 150), (3, 0)))])
    assert b.get(ea.F_SOLID)[150:154, 200:205].all()
    b.clear_bodies()
    for fld, _ in MASKS:
        assert_bits(b.get(fld), a.get(fld), "field %d behind set and clear" % fld)
    launches = lambda s: {k: v[1] for k, v in s.profile().items()}
    # The two calls are mask edits (docs/stage_validity.md: eu_vd_masks_changed), so b's first substep rebuilds what an edit invalidates - the column-major
    # sink | solid grid of the marker stage, one launch of k_blocked_transpose in the class SETTLE_EXTRA names - and runs the full forms of the lean passes, which
    # are other instantiations of the same launches.  That one difference is pinned exactly; from the second frame on the counts per class are the same.
    a.profile_reset(); b.profile_reset()
    a.step(); b.step()
    la, lb = launches(a), launches(b)
    extra = {k: lb.get(k, 0) - la.get(k, 0) for k in set(la) | set(lb) if lb.get(k, 0) != la.get(k, 0)}
    print("launches of the first frame behind set and clear, b - a:", extra)
    assert extra == SETTLE_EXTRA
    a.profile_reset(); b.profile_reset()
    for k in range(8):
        a.step(); b.step()
    assert launches(a) == launches(b)
    for fld in STATE_FIELDS:
        assert_bits(b.get(fld), a.get(fld), "field %d" % fld)
    assert a.stats().rng_state == b.stats().rng_state
    a.close(); b.close()


def test_a_body_at_rest_is_an_edited_wall():
    box = (12, 2, 14, 9)
    for opts in ((), ((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1))):
        a = ea.Simulation(96, 64).load_text(scenarios.dam_break(), upscale=True)
        b = ea.Simulation(96, 64).load_text(scenarios.dam_break(), upscale=True)
        for k, v in opts:
            a.set_option(k, v); b.set_option(k, v)
        a.set_bodies([record(bref.body((3, 8), (12.0, 2.0), (0.0, 0.0), (0.25, 0.0), 0.0, 1.0))])
        b.edit_box(ea.EDIT_SOLID, box)
        for k in range(30):
            a.step(); b.step()
            if k % 5 == 4:
                for fld in STATE_FIELDS + (ea.F_SOLID,):
                    assert_bits(a.get(fld), b.get(fld), "frame %d field %d" % (k, fld))
        assert np.abs(a.get(ea.F_U)).max() > 0.5 and a.stats().rng_state == b.stats().rng_state
        a.close(); b.close()


def _body_run(size, start, frames, bodies, options=()):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50).load_text(scenarios.dam_break(), upscale=True)
    for key, val in options:
        sim.set_option(key, val)
    for _ in range(start):
        sim.step()
    sim.time = 0.0
    sim.set_bodies([record(b) for b in bodies])
    out = []
    for _ in range(frames):
        sim.step()
        out.append([sim.get(fld) for fld in STATE_FIELDS + (ea.F_SOLID,)])
    sim.close()
    return out


def test_lean_forms_give_the_bits_of_the_full_ones():
    """a piston shifts through the spreading dam break while tiles fall dry and others get wet (asserted below): the tile map's readers against the full passes"""
    size = (264, 136)
    bodies = [bref.body((4, 60), (3, 2), (10, 0))]
    lean = _body_run(size, 30, 60, bodies)
    count = STATE_FIELDS.index(ea.F_COUNT)
    solid = len(STATE_FIELDS)
    assert lean[-1][solid][10:60, 30:64].all(axis=0).sum() == 4 and not lean[0][solid][10:60, 30:64].any()      # the piston has come a long way
    full = _body_run(size, 30, 60, bodies, options=((ea.OPT_NO_TILE_MAP, 1), (ea.OPT_VELOCITY_TWO_PASS, 1), (ea.OPT_MARKERS_TWO_PASS, 1), (ea.OPT_BUILD_TWO_PASS, 1)))
    for k, (a, b) in enumerate(zip(lean, full)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert_bits(x, y, "frame %d field %d" % (k, j))
    dried = [tuple(t) for t in np.argwhere([[not lean[-1][count][64 * j:64 * j + 64, 64 * i:64 * i + 64].any() and lean[0][count][64 * j:64 * j + 64, 64 * i:64 * i + 64].any()
                                             for i in range(5)] for j in range(3)])]
    wetted = [tuple(t) for t in np.argwhere([[lean[-1][count][64 * j:64 * j + 64, 64 * i:64 * i + 64].any() and not lean[0][count][64 * j:64 * j + 64, 64 * i:64 * i + 64].any()
                                              for i in range(5)] for j in range(3)])]
    assert dried and wetted, (dried, wetted)


# ----------------------------------------------------------------------------- the piston's known answer on the device
@pytest.mark.parametrize("precond", [ea.PRECOND_IC0_TILE, ea.PRECOND_IC0_TILE_MG])
@pytest.mark.parametrize("vx", [4.0, 0.75])
def test_a_piston_drives_wx_times_its_face_through_every_section(precond, vx):
    X, Y = PISTON_GRID
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=precond, max_iterations=PISTON_CAP).load_text(channel_text(X, Y))
    sim.set_bodies([record(piston(vx))])
    assert origins_of(sim) == [[PISTON_X, CH_Y0]]
    dt = float(F32(0.05))
    zero = np.zeros((Y, X), F32)
    sim.set(ea.F_UTMP, zero); sim.set(ea.F_VTMP, zero)
    sim.stage(ea.STAGE_PROJECT, dt)
    st = sim.stats()
    tol = 1e-6      # euler_config.tol's default, (double)1e-6f
    assert 0 < st.last_pcg_iterations < PISTON_CAP and st.last_residual <= float(np.float64(F32(1e-6)))      # converged
    p = sim.get(ea.F_PRESSURE)
    assert (p >= 0).all() and p.max() > 0
    piston_sections(sim.get(ea.F_U), sim.get(ea.F_V), p, sim.get(ea.F_SOLID), sim.get(ea.F_COUNT), [PISTON_X, CH_Y0], F32(vx), dt,
                    float(np.float64(F32(tol))), st.last_pcg_iterations)
    assert not sim.get(ea.F_UTMP).any() and not sim.get(ea.F_VTMP).any()
    sim.close()


# ----------------------------------------------------------------------------- the surface
def test_refusals_in_order_the_edit_next_to_a_body_and_the_loads(tmp_path):
    X, Y = 96, 64
    sim = ea.Simulation(X, Y)
    L = sim.L
    good = ea.bodies_array([record(bref.body((4, 6), (20, 20), (4, 0))), record(bref.body((3, 3), (50, 30), (0, 0), (1.0, 0.5), 1.0))])

    def call(s, b=good, n=None):
        return L.euler_set_bodies(s.h if s else None, b.ctypes.data if b is not None else None, len(b) if n is None else n)

    def bad(at, **kw):
        b = good.copy()
        for k, v in kw.items():
            b[k][at] = v
        return b

    assert call(None) == EULER_EINVAL                                                              # 1: a null handle
    assert call(sim, bad(0, reserved=(1, 0), x=np.nan), n=99) == EULER_ESTATE                      # 3: nothing loaded, in front of the list
    sim.load_text(scenarios.dam_break(), upscale=True)
    before = sim.hbm_bytes()
    state = [sim.get(fld) for fld in STATE_FIELDS + (ea.F_SOLID, ea.F_SOURCE, ea.F_SINK)]
    assert call(sim, n=-1) == EULER_EINVAL and b"bodies (0" in L.euler_last_error()                # 4
    assert call(sim, bad(0, reserved=(1, 0)), n=17) == EULER_EINVAL and b"bodies (0" in L.euler_last_error()
    assert call(sim, None, n=2) == EULER_EINVAL and b"null" in L.euler_last_error()
    order = [(bad(1, reserved=(0, 5), x=np.nan, w=0, hz=-1, vx=50), b"body 1: reserved"),         # 5, in this order
             (bad(1, x=np.nan, w=0, hz=-1, vx=50), b"body 1: a value"), (bad(0, phase=np.inf), b"body 0: a value"), (bad(0, amp_y=-np.inf), b"body 0: a value"),
             (bad(1, w=0, hz=-1, vx=50), b"body 1: 0 x 3"), (bad(0, w=X - 3), b"body 0:"), (bad(0, h=Y - 3), b"body 0:"), (bad(1, h=-2), b"body 1:"),
             (bad(1, hz=-1e-3, vx=50), b"body 1: hz"), (bad(1, vx=10.5), b"body 1: a speed"), (bad(0, vy=-10.5), b"body 0: a speed"),
             (bad(1, amp_x=1.6), b"body 1: a speed"), (bad(1, amp_y=-1.6), b"body 1: a speed")]
    for b, word in order:
        assert call(sim, b) == EULER_EINVAL and word in L.euler_last_error(), (word, L.euler_last_error())
    both = bad(1, reserved=(1, 1))
    both["vx"][0] = 11
    assert call(sim, both) == EULER_EINVAL and b"body 0: a speed" in L.euler_last_error()           # the first bad body is the one named
    # a refused call changes and allocates nothing
    assert sim.hbm_bytes() == before and len(sim.bodies()[0]) == 0
    for fld, a in zip(STATE_FIELDS + (ea.F_SOLID, ea.F_SOURCE, ea.F_SINK), state):
        assert_bits(sim.get(fld), a, "field %d" % fld)
    # set: the records come back, the rectangles are solid; no device buffer at all
    assert call(sim) == 0 and sim.hbm_bytes() == before
    got, now = sim.bodies()
    assert got.tobytes() == good.tobytes() and [(int(s["ox"]), int(s["oy"])) for s in now] == [(20, 20), (50, 30)]
    solid = sim.get(ea.F_SOLID)
    assert solid[20:26, 20:24].all() and solid[30:33, 50:53].all() and not sim.get(ea.F_COUNT)[20:26, 20:24].any()
    n = C.c_int32(-1)
    assert L.euler_get_bodies(sim.h, None, 0, None, C.byref(n)) == 0 and n.value == 2
    assert L.euler_get_bodies(sim.h, got.ctypes.data, 1, None, C.byref(n)) == EULER_EINVAL and L.euler_get_bodies(sim.h, None, 0, None, None) == EULER_EINVAL
    assert call(sim, bad(0, vx=np.nan)) == EULER_EINVAL and sim.bodies()[0].tobytes() == good.tobytes()      # a refusal leaves the list as set
    # euler_edit_box: refused on a body's rectangle, accepted beside it
    for box in ((20, 20, 23, 25), (23, 25, 30, 30), (10, 10, 20, 20), (22, 22, 22, 22), (1, 1, X - 2, Y - 2), (52, 32, 60, 40)):
        for op in (ea.EDIT_SOLID, ea.EDIT_CLEAR, ea.EDIT_FILL):
            assert L.euler_edit_box(sim.h, op, *box) == EULER_ESTATE and b"body" in L.euler_last_error(), box
    assert_bits(sim.get(ea.F_SOLID), solid, "solid behind the refused edits")
    for box in ((24, 20, 30, 25), (20, 26, 23, 30), (16, 20, 19, 25), (20, 14, 23, 19), (53, 30, 60, 40)):
        assert L.euler_edit_box(sim.h, ea.EDIT_SOLID, *box) == 0, box
    # replacing the list opens the old rectangles; n = 0 removes the bodies
    one = ea.bodies_array([record(bref.body((2, 2), (70, 40)))])
    assert call(sim, one) == 0
    solid = sim.get(ea.F_SOLID)
    assert not solid[20:26, 20:24].any() and not solid[30:33, 50:53].any() and solid[40:42, 70:72].all()
    assert L.euler_set_bodies(sim.h, None, 0) == 0 and len(sim.bodies()[0]) == 0 and not sim.get(ea.F_SOLID)[40:42, 70:72].any()
    assert L.euler_edit_box(sim.h, ea.EDIT_SOLID, 70, 40, 71, 41) == 0
    # a load drops the bodies: scenario and snapshot
    assert call(sim) == 0
    snap = str(tmp_path / "state.snap")
    sim.save_state(snap)
    sim.load_state(snap)
    assert len(sim.bodies()[0]) == 0 and sim.get(ea.F_SOLID)[20:26, 20:24].all()      # their cells are whatever the loaded masks say
    assert L.euler_edit_box(sim.h, ea.EDIT_CLEAR, 20, 20, 23, 25) == 0
    assert call(sim) == 0
    sim.load_text(scenarios.dam_break(), upscale=True)
    assert len(sim.bodies()[0]) == 0 and not sim.get(ea.F_SOLID)[20:26, 20:24].any()
    with pytest.raises(ea.EulerError) as e:
        sim.set_bodies([record(bref.body((4, 6), (20, 20), (40, 0)))])
    assert e.value.code == EULER_EINVAL and "body 0" in str(e.value)
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    assert call(slab, bad(0, reserved=(1, 0))) == EULER_ESTATE and b"slab" in L.euler_last_error()      # 2: in front of "nothing loaded" and of the list
    slab.close()


# ----------------------------------------------------------------------------- the front end
CLI_BODIES = [bref.body((3, 20), (6, 2), (6, 0)), bref.body((2, 10), (60, 2), (0, 0), (3, 0), 0.5, np.pi / 6)]
CLI_FLAGS = ["--body", "3,20:6,2:6,0", "--body", "2,10:60,2:0,0:3,0:0.5:30"]


def test_cli_bodies(tmp_path):
    X, Y = 100, 40
    text = scenarios.dam_break()
    scn = tmp_path / "dam.txt"
    scn.write_text(text)
    base = [EXE, "--dump", "--window", "98x38", "--size", "%dx%d" % (X, Y), "--upscale"]

    def run(*flags, frames=20):
        r = subprocess.run(base + ["--frames", str(frames)] + list(flags) + [str(scn)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    def driven(frames, gravity=None, edit=None):
        sim = ea.Simulation(X, Y).load_text(text, upscale=True)
        if gravity:
            sim.set_forcing(gravity)
        bodies = [record(b) for b in CLI_BODIES]
        bodies[1]["phase"] = 30.0 * (3.14159265358979323846 / 180.0)      # the command's own conversion
        sim.set_bodies(bodies)
        out = [sim.draw(98, 38)]
        for k in range(1, frames + 1):
            if edit and edit[0] == k:
                sim.edit_box(edit[1], edit[2])
            sim.step()
            out.append(sim.draw(98, 38))
        sim.close()
        return out

    want = driven(20)
    assert dumped_frames(run(*CLI_FLAGS)) == want and len(set(want)) > 15
    assert dumped_frames(run(*CLI_FLAGS, "--gravity", "3,-8", frames=8)) == driven(8, gravity=(3, -8))
    assert dumped_frames(run(*CLI_FLAGS, "--edit", "3:solid:40,2,42,20", frames=8)) == driven(8, edit=(3, ea.EDIT_SOLID, (40, 2, 42, 20)))
    # with the other modes: the run goes through, and differs from the one without bodies
    for extra in (["--fit", "--ppm", str(tmp_path / "p_"), "--ppm-every", "5", "--gauge", "level:2,1,4,38", "--gauges", str(tmp_path / "g.csv"), "--heat", "1:0.5"],
                  ["--view", "5,3,60,30", "--maccormack", "--advection", "rk2"]):
        assert run(*CLI_FLAGS, *extra, frames=6) != run(*extra, frames=6), extra
    # a run without the flag is byte for byte what it was
    sim = ea.Simulation(X, Y).load_text(text, upscale=True)
    plain = [sim.draw(98, 38)]
    for k in range(3):
        sim.step()
        plain.append(sim.draw(98, 38))
    sim.close()
    assert dumped_frames(run(frames=3)) == plain
    # usage errors and refused values: status 1, nothing on stdout
    many = []
    for k in range(17):
        many += ["--body", "1,1:%d,5:0,0" % (3 + 2 * k)]
    for bad_flags, word in ((["--body", "3,20"], b"--body W,H"), (["--body", "3,20:6,2:6"], b"--body W,H"), (["--body", "3,20:6,2:6,0x"], b"--body W,H"),
                            (["--body", "3,20:6,2:6,0:1,0"], b"--body W,H"), (["--body", "3,20:6,2:6,0:1,0:0.5:30:1"], b"--body W,H"), (many, b"--body W,H"),
                            (["--body", "3,20:6,2:60,0"], b"speed"), (["--body", "0,20:6,2:6,0"], b"body 0"), (["--body", "3,20:6,2:0,0:1,0:-1"], b"hz"),
                            (CLI_FLAGS + ["--edit", "2:solid:5,2,30,10"], b"body")):
        r = subprocess.run(base + ["--frames", "3"] + bad_flags + [str(scn)], capture_output=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (bad_flags, r.stderr)
    assert run(*many[:32], frames=2)      # 16 are taken
