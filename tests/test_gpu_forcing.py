"""euler_set_forcing on the GPU (docs/forcing.md): gravity vector, shaken tank and force boxes against the test-side restatement (tests/forcing_ref.py, pinned
on the CPU by test_forcing_host.py), bit for bit in the parity mode (every grid here has fewer than 65 536 cells): the velocity stage teacher-forced under
each transport and with viscosity, free runs, the known answers of the host test on the device, the default record as today's path, the lean forms against
the full ones, the forcing next to an edit, the gauges, between substeps and between stages, the refusals and the clock, and `euler --gravity / --shake / --force`.
The (ax, ay) of the restatement are euler_forcing_at's own, so no libm difference reaches these tests."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import edit_ref as eref
import euler_amd as ea
import forcing_ref as fref
import gauges_ref as gref
from euler_amd import scenarios
from observer_util import EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames, no_trace_pair
from oracle_lib import Oracle
from test_forcing_host import FALL_BOX, PUMP, WEIGHT_CAP, WEIGHT_TOL, block_text, free_fall_check, pump_flux, weight_bound
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

GRIDS = [(100, 40),      # one band
         (103, 41),      # odd width
         (264, 136),     # three bands, several tiles, dry tiles
         (1031, 70)]     # seventeen tile columns, two bands
DYE = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B)
DYE_TMP = (ea.F_DYE_RTMP, ea.F_DYE_GTMP, ea.F_DYE_BTMP)
GRAVITY, SHAKE = (3.0, -8.0), (1.5, 0.5, 0.8, 0.3)
TIMES = (0.0, 0.37, 12.5)
TRANSPORTS = ((0, 0), (1, 0), (0, 1), (1, 1))      # (rk2, maccormack)


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("forcing_gpu"))


def record(f, nboxes=0):
    return ea.forcing_record((f["gx"], f["gy"]), (f["shake_x"], f["shake_y"], f["shake_hz"], f["shake_phase"]), nboxes)


def acc_at(f, t):
    """the uniform acceleration as the library itself forms it"""
    return ea.forcing_at(record(f), t)


def dry_box(count):
    """a box inside a 64 x 64 tile without a marker whose right and upper neighbours have none either; else a box in the air"""
    Yg, Xg = count.shape
    wet = lambda tx, ty: count[ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64].any()
    for ty in range((Yg + 63) // 64):
        for tx in range((Xg + 63) // 64):
            if not (wet(tx, ty) or wet(tx + 1, ty) or wet(tx, ty + 1)):
                x0, y0, x1, y1 = max(tx * 64 + 3, 1), max(ty * 64 + 2, 1), min(tx * 64 + 40, Xg - 2), min(ty * 64 + 30, Yg - 2)
                if x0 <= x1 and y0 <= y1:
                    return (x0, y0, x1, y1)
    return (Xg - 12, Yg - 8, Xg - 6, Yg - 4)


def boxes_of(Xg, Yg, count):
    """seven boxes: two that overlap, the first of them again, one across x = 63 | 64 and y = 63 | 64 (clipped to the interior), one in a dry tile, one touching
    X - 2 and Y - 2, one of a single cell"""
    xi, yi = Xg - 2, Yg - 2
    clip = lambda b: (min(b[0], xi), min(b[1], yi), min(b[2], xi), min(b[3], yi))
    return [((10, 3, 30, 12), (4.0, -1.5)), ((20, 8, 40, 16), (-2.25, 3.0)), ((10, 3, 30, 12), (4.0, -1.5)), (clip((60, 60, 70, 70)), (0.7, 0.9)),
            (dry_box(count), (5.0, 5.0)), ((xi - 4, yi - 3, xi, yi), (-3.0, 0.0)), ((5, 6, 5, 6), (0.0, 1e4))]


def set_forcing(sim, f, boxes):
    sim.set_forcing((f["gx"], f["gy"]), (f["shake_x"], f["shake_y"], f["shake_hz"], f["shake_phase"]), boxes)


def compare_state(o, sim, what):
    for fld, want, n in ((ea.F_U, o.u, "u"), (ea.F_V, o.v, "v"), (ea.F_COUNT, o.count, "count"), (ea.F_PREV_COUNT, o.prev_count, "prev_count"), (ea.F_MARKERS, o.markers, "markers")):
        assert_bits(sim.get(fld), want, "%s %s" % (what, n))


def pair(size, text=None, **kw):
    text = text or scenarios.dam_break()
    sim = ea.Simulation(*size, **kw).load_text(text, upscale=True)
    o = Oracle(*size, rainbow=bool(kw.get("rainbow"))).load_text(text, upscale=True)
    o.c.viscosity = kw.get("viscosity", 0.0)
    return sim, o


# ----------------------------------------------------------------------------- the stage, teacher-forced
def _front_half(sim, o, dt):
    """the stages in front of STAGE_ADVECT_VELOCITY on both sides"""
    lib = o.lib
    sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
    lib.eo_advect_markers(o.ptr, C.c_float(dt))
    sim.stage(ea.STAGE_REFRESH_COUNTS)
    lib.eo_refresh_marker_counts(o.ptr)
    sim.stage(ea.STAGE_SOURCES)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            lib.eo_extrapolate(o.ptr, o.f32p(q), 0)
    lib.eo_update_fluid_sources(o.ptr)
    sim.stage(ea.STAGE_EXTRAPOLATE)
    for q, t in ((o.u, 1), (o.v, 2)):
        lib.eo_extrapolate(o.ptr, o.f32p(q), t)
    for q, t in ((o.u, 1), (o.v, 2)):
        lib.eo_zero_bounds(o.ptr, o.f32p(q), t)
    assert_bits(sim.get(ea.F_U), o.u, "u in front of the advection")
    assert_bits(sim.get(ea.F_COUNT), o.count, "count in front of the advection")


def _stage_cases(am, size, frame, viscosity, transports):
    sim, o = pair(size, rainbow=True, viscosity=viscosity)
    for _ in range(frame):
        sim.step(); o.step()
    dt = sim.timestep(0.1)
    assert dt == o.timestep(0.1)
    _front_half(sim, o, dt)
    f = fref.forcing(GRAVITY, SHAKE)
    boxes = boxes_of(*size, np.array(o.count))
    names = ("u", "v", "utmp", "vtmp", "cr", "cg", "cb", "crtmp", "cgtmp", "cbtmp")
    fields = (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP) + DYE + DYE_TMP
    for n, fld in zip(names[4:], fields[4:]):      # (the tmp fields of the dye hold what the device left there)
        getattr(o, n)[...] = sim.get(fld)
    keep = {n: np.array(getattr(o, n)) for n in names}
    touched = 0
    for k, (rk2, mc) in enumerate(transports):
        sim.set_option(ea.OPT_ADVECT_RK2, rk2)
        sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
        for t in TIMES if k == 0 else (TIMES[k % 3],):
            for n, fld in zip(names, fields):
                getattr(o, n)[...] = keep[n]
                sim.set(fld, keep[n])
            set_forcing(sim, f, boxes)
            sim.time = t
            sim.stage(ea.STAGE_ADVECT_VELOCITY, dt)
            assert sim.time == t      # a stage is not a substep
            fref.advect_velocity_stage(am, o, dt, f, boxes, t, rk2, mc, acc=acc_at(f, t))
            what = "%dx%d frame %d rk2=%d mc=%d nu=%g t=%g" % (size + (frame, rk2, mc, viscosity, t))
            assert_bits(sim.get(ea.F_UTMP), o.utmp, what + " utmp")
            assert_bits(sim.get(ea.F_VTMP), o.vtmp, what + " vtmp")
            for fld, q in zip(DYE, (o.cr, o.cg, o.cb)):      # the dye is untouched by the forcing: what the transport alone leaves
                assert_bits(sim.get(fld), q, "%s dye %d" % (what, fld))
            lu, lv = fref.live_faces(o.solid, o.count)
            assert not o.utmp[~lu].any() and not o.vtmp[~lv].any()      # a face that is not live stays 0
            touched += int(lu.sum())
    assert touched > 0
    sim.close(); o.close()


@pytest.mark.parametrize("frame", [0, 6])
@pytest.mark.parametrize("size", GRIDS)
def test_stage_teacher_forced_under_each_transport(am, size, frame):
    _stage_cases(am, size, frame, 0.0, TRANSPORTS)


def test_stage_teacher_forced_with_viscosity(am):
    _stage_cases(am, (264, 136), 6, 0.5, ((0, 0), (1, 1)))


# ----------------------------------------------------------------------------- free runs
def _free_run(am, size, frames, options=(), rk2=0, mc=0, boxes=None, **kw):
    """-> the per-frame states of the device run (the fields of STATE_FIELDS), compared against the composition frame by frame"""
    sim, o = pair(size, **kw)
    for key, val in options:
        sim.set_option(key, val)
    sim.set_option(ea.OPT_ADVECT_RK2, rk2)
    sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
    f = fref.forcing(GRAVITY, SHAKE)
    boxes = boxes_of(*size, np.array(o.count)) if boxes is None else boxes
    set_forcing(sim, f, boxes)
    clock = fref.Clock()
    out = []
    for k in range(frames):
        sim.step()
        n, it = fref.step(am, o, f, boxes, clock, rk2, mc, acc_at)
        st = sim.stats()
        assert (st.last_substeps, st.last_pcg_iterations) == (n, it), (size, k)
        compare_state(o, sim, "%dx%d frame %d" % (size + (k,)))
        assert sim.time == clock.t, (k, sim.time, clock.t)      # exactly
        out.append([sim.get(fld) for fld in STATE_FIELDS])
    assert np.abs(o.u).max() > 1 and clock.t > 0
    sim.close(); o.close()
    return out


@pytest.mark.parametrize("size", [(100, 40), (264, 136)])
def test_free_run_against_the_composition(am, size):
    _free_run(am, size, 20)


def test_free_run_with_maccormack_and_rk2(am):
    _free_run(am, (100, 40), 8, rk2=1, mc=1)


# The lean-forms run starts where the dam break is about to enter new ground: 26 unforced frames in, the front runs along the floor towards the tile (3, 0) -
# columns 192 .. 255, rows 0 .. 63 -, which holds no marker then and some ten forced frames later.  LATE_BOX lies in that tile.  (From frame 0 the block takes
# 25 frames to reach the floor: no tile of this grid changes in 20 frames.)  The test asserts what it needs: dry at the run's frame 0, wet by its frame 10.
LATE_START = 26
LATE_BOX = ((195, 3, 250, 20), (-6.0, 2.0))


def _device_run(size, start, frames, boxes, options=()):
    """`start` unforced frames, then `frames` forced ones -> the count grid at the start of the forced run and the per-frame states behind it"""
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50).load_text(scenarios.dam_break(), upscale=True)      # (one launch per solve: quick)
    for key, val in options:
        sim.set_option(key, val)
    for _ in range(start):
        sim.step()
    c0 = sim.get(ea.F_COUNT)
    set_forcing(sim, fref.forcing(GRAVITY, SHAKE), boxes)
    out = []
    for _ in range(frames):
        sim.step()
        out.append([sim.get(fld) for fld in STATE_FIELDS])
    sim.close()
    return c0, out


def test_lean_forms_give_the_bits_of_the_full_ones():
    size = (264, 136)
    (x0, y0, x1, y1), _ = LATE_BOX
    tx, ty = x0 // 64, y0 // 64
    assert x1 // 64 == tx and y1 // 64 == ty      # one tile
    tile = (slice(ty * 64, ty * 64 + 64), slice(tx * 64, tx * 64 + 64))
    boxes = boxes_of(*size, np.zeros((size[1], size[0]), np.uint8))[:6] + [LATE_BOX]
    c0, lean = _device_run(size, LATE_START, 20, boxes)
    assert not c0[tile].any()                                            # dry at the run's frame 0
    assert lean[9][STATE_FIELDS.index(ea.F_COUNT)][tile].any()           # ... and wet by its frame 10
    (bx0, by0, bx1, by1), _ = LATE_BOX
    assert lean[19][STATE_FIELDS.index(ea.F_COUNT)][by0:by1 + 1, bx0:bx1 + 1].any()      # the box has water to push
    c1, full = _device_run(size, LATE_START, 20, boxes, options=((ea.OPT_NO_TILE_MAP, 1), (ea.OPT_VELOCITY_TWO_PASS, 1), (ea.OPT_MARKERS_TWO_PASS, 1), (ea.OPT_BUILD_TWO_PASS, 1)))
    assert_bits(c1, c0, "count at the start")
    for k, (a, b) in enumerate(zip(lean, full)):
        for fld, x, y in zip(STATE_FIELDS, a, b):
            assert_bits(x, y, "frame %d field %d" % (k, fld))


# ----------------------------------------------------------------------------- the known answers of the host test, on the device
def test_free_fall_is_exact():
    sim = ea.Simulation(64, 40).load_text(block_text(64, 40, FALL_BOX))
    dt = sim.timestep(0.1)
    assert np.float32(dt) == np.float32(0.1)
    sim.set_forcing((3, -7))
    sim.substep(dt)
    assert sim.stats().last_pcg_iterations == 0 and sim.time == float(np.float32(dt))
    free_fall_check(sim.get(ea.F_U), sim.get(ea.F_V), sim.get(ea.F_SOLID), sim.get(ea.F_COUNT), dt)
    sim.close()


@pytest.mark.parametrize("size", [(64, 40), (100, 70)])
@pytest.mark.parametrize("gy", [-5.0, -20.0])
def test_weight_scales_with_gravity(size, gy):
    Xg, Yg = size
    sim = ea.Simulation(Xg, Yg, tol=WEIGHT_TOL, max_iterations=WEIGHT_CAP).load_half_tank()      # (the tolerance: test_forcing_host.py)
    sim.set_forcing((0, gy))
    sim.substep(sim.timestep(0.1))
    assert sim.stats().last_pcg_iterations < WEIGHT_CAP
    rec = sim.gauges([(ea.GAUGE_FORCE, (1, 1, Xg - 2, Yg - 2))])[0]
    weight_bound(rec, gy)
    sim.close()


def test_no_force_no_motion():
    sim = ea.Simulation(64, 40).load_half_tank()
    m0, c0 = sim.get(ea.F_MARKERS), sim.get(ea.F_COUNT)
    sim.set_forcing((0, 0))
    for _ in range(5):
        sim.step()
    assert not sim.get(ea.F_U).view(np.uint32).any() and not sim.get(ea.F_V).view(np.uint32).any()
    assert_bits(sim.get(ea.F_MARKERS), m0, "markers")
    assert_bits(sim.get(ea.F_COUNT), c0, "count")
    sim.close()


def test_a_pump_drives_a_current():
    sim = ea.Simulation(64, 40).load_half_tank()
    sim.set_forcing(boxes=[PUMP])
    for _ in range(5):
        sim.step()
    assert pump_flux(sim.get(ea.F_SOLID), sim.get(ea.F_COUNT), sim.get(ea.F_U), sim.get(ea.F_V)) > 0
    sim.close()


# ----------------------------------------------------------------------------- the default record is today's path
def _default_pair(options=(), **kw):
    def make():
        s = ea.Simulation(264, 136, **kw)
        for k, v in options:
            s.set_option(k, v)
        return s.load_text(scenarios.dam_break(), upscale=True)

    def look(s, stepped):      # before and after every frame, and between the stages of a substep
        s.set_forcing()
        f, b = s.forcing()
        assert f.tobytes() == ea.forcing_default().tobytes() and len(b) == 0

    for s in no_trace_pair(make, look, None, STATE_FIELDS, 20, compare_every=5):
        s.close()


def test_the_default_record_is_todays_path():
    _default_pair(dot_mode=ea.DOT_SEQUENTIAL)


def test_the_default_record_with_maccormack_and_rk2():
    _default_pair(options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)), dot_mode=ea.DOT_SEQUENTIAL)


def test_the_default_record_with_the_tile_solver():
    _default_pair(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE)


def test_back_to_the_default_record_is_todays_path():
    """a handle that was forced for a while and then set back runs on as one that was handed the same state"""
    a = ea.Simulation(100, 40).load_text(scenarios.dam_break(), upscale=True)
    b = ea.Simulation(100, 40).load_text(scenarios.dam_break(), upscale=True)
    a.set_forcing((2, -6), (1, 1, 2.0), [((10, 3, 30, 12), (4.0, -1.5))])
    for _ in range(4):
        a.step()
    a.set_forcing()
    for fld in (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP, ea.F_COUNT, ea.F_PREV_COUNT):
        b.set(fld, a.get(fld))
    b.set_markers(a.get(ea.F_MARKERS))
    for k in range(6):
        a.step(); b.step()
        for fld in (ea.F_U, ea.F_V, ea.F_COUNT, ea.F_MARKERS):
            assert_bits(a.get(fld), b.get(fld), "frame %d field %d" % (k, fld))
    a.close(); b.close()


# ----------------------------------------------------------------------------- neighbours
def test_a_forced_step_behind_an_edit_and_behind_the_gauges(am):
    size = (264, 136)
    sim, o = pair(size)
    f = fref.forcing(GRAVITY, SHAKE)
    boxes = boxes_of(*size, np.array(o.count))
    set_forcing(sim, f, boxes)
    clock = fref.Clock()
    for k in range(8):
        if k == 3:      # a wall through the two overlapping force boxes, the markers in it gone
            wall = (18, 2, 24, 20)
            sim.edit_box(ea.EDIT_SOLID, wall)
            sl = (slice(wall[1], wall[3] + 1), slice(wall[0], wall[2] + 1))
            o.solid[sl], o.source[sl], o.sink[sl] = 1, 0, 0
            o.set_markers(eref.delete_in_box_vectorised(o.markers, wall))
            o.count[sl] = 0
        if k == 5:
            sim.gauges([(ea.GAUGE_FLUX, (20, 1, 20, 60)), (ea.GAUGE_FORCE, (1, 1, 262, 134)), (ea.GAUGE_LEVEL, (1, 1, 262, 134))])
        sim.step()
        fref.step(am, o, f, boxes, clock, acc_at=acc_at)
        compare_state(o, sim, "frame %d" % k)
    assert sim.time == clock.t
    sim.close(); o.close()


def test_a_forcing_changed_between_substeps_and_between_stages(am):
    size = (103, 41)
    sim, o = pair(size)
    for _ in range(5):
        sim.step(); o.step()
    boxes = boxes_of(*size, np.array(o.count))
    f1, f2, f3 = fref.forcing(GRAVITY, SHAKE), fref.forcing((-4.0, 2.0)), fref.forcing((0.0, -10.0), (0.0, 3.0, 5.0, 1.0))
    clock = fref.Clock()
    sim.time = clock.t = 2.5
    for f, bx in ((f1, boxes), (f2, boxes[:2]), (f3, [])):      # three substeps of at most 0.03 s, as one frame would cut them, a forcing each
        set_forcing(sim, f, bx)
        dt = sim.timestep(0.03)
        assert dt == o.timestep(0.03) and 0 < dt <= 0.03
        sim.substep(dt)
        fref.substep(am, o, dt, f, bx, clock, acc_at=acc_at)
        compare_state(o, sim, "substep under %r" % (f,))
        assert sim.time == clock.t
    # between stages: the forcing the velocity stage finds is the one that counts, and the clock stands still
    dt = sim.timestep(0.1)
    assert dt == o.timestep(0.1)
    t = sim.time
    for st in range(6):
        set_forcing(sim, f1 if st == ea.STAGE_ADVECT_VELOCITY else f3, boxes if st == ea.STAGE_ADVECT_VELOCITY else [])
        sim.stage(st, dt)
    assert sim.time == t
    fref.substep(am, o, dt, f1, boxes, fref.Clock(t), acc_at=acc_at)
    compare_state(o, sim, "forcing set between stages")
    sim.close(); o.close()


# ----------------------------------------------------------------------------- the surface
def test_refusals_in_order_the_buffer_and_the_clock(tmp_path):
    X, Y = 264, 136
    sim = ea.Simulation(X, Y)
    L = sim.L
    good = ea.forcing_record(GRAVITY, SHAKE, 2)
    gb = np.zeros(2, ea.FORCE_BOX_DTYPE)
    gb[0], gb[1] = (10, 3, 30, 12, 4.0, -1.5), (60, 60, 70, 70, 0.5, 0.5)

    def call(s, f=good, b=gb):
        return L.euler_set_forcing(s.h if s else None, f.ctypes.data if f is not None else None, b.ctypes.data if b is not None else None)

    def bad(**kw):
        f = good.copy()
        for k, v in kw.items():
            f[k] = v
        return f

    assert call(None) == EULER_EINVAL and call(sim, f=None) == EULER_EINVAL                                    # 1: a null argument
    assert call(sim, f=bad(reserved=1, gx=np.nan)) == EULER_ESTATE                                            # 3: nothing loaded, in front of the record
    assert sim.time == 0.0
    sim.load_text(scenarios.dam_break(), upscale=True)
    before = sim.hbm_bytes()
    state = [sim.get(fld) for fld in STATE_FIELDS]
    order = [(bad(reserved=1, gx=np.nan, shake_hz=-1, nboxes=99), b"reserved"), (bad(reserved2=0.5, gy=np.inf), b"reserved"),                      # 4
             (bad(gx=np.nan, shake_hz=-1, nboxes=99), b"gravity"), (bad(gy=-10000.5), b"gravity"), (bad(shake_x=np.inf), b"shake"), (bad(shake_y=2e4), b"shake"),      # 5
             (bad(shake_hz=-1e-3, nboxes=99), b"shake_hz"), (bad(shake_hz=np.inf), b"shake_hz"), (bad(shake_phase=np.nan), b"shake_phase"),         # 6
             (bad(nboxes=-1), b"boxes"), (bad(nboxes=65), b"boxes")]                                                                                # 7
    for f, word in order:
        assert call(sim, f=f) == EULER_EINVAL and word in L.euler_last_error(), (f, L.euler_last_error())
    assert call(sim, b=None) == EULER_EINVAL and b"null" in L.euler_last_error()
    for at in (0, 1):
        for field, val, word in (("fx", np.nan, "force"), ("fy", -1.5e4, "force"), ("x0", 0, "["), ("y0", 0, "["), ("x1", X - 1, "["), ("y1", Y - 1, "["), ("x0", 80, "["), ("y0", 90, "[")):
            wb = gb.copy()
            wb[field][at] = val
            assert call(sim, b=wb) == EULER_EINVAL and ("box %d: %s" % (at, word)).encode() in L.euler_last_error(), (at, field, L.euler_last_error())
    wb = gb.copy()
    wb["x0"][0], wb["fy"][1] = 0, np.nan
    assert call(sim, b=wb) == EULER_EINVAL and b"box 1: force" in L.euler_last_error()      # a value comes in front of any box's place
    wb["fy"][1], wb["y1"][1] = 0, Y
    assert call(sim, b=wb) == EULER_EINVAL and b"box 0: [" in L.euler_last_error()          # the first box refused is the one named
    # a refused call changes and allocates nothing
    assert sim.hbm_bytes() == before
    f, b = sim.forcing()
    assert f.tobytes() == ea.forcing_default().tobytes() and len(b) == 0
    for fld, a in zip(STATE_FIELDS, state):
        assert_bits(sim.get(fld), a, "field %d" % fld)
    # the buffer: 64 boxes of 24 bytes, 16 per touched tile; kept, grown, counted; no buffer without boxes
    assert call(sim, f=bad(nboxes=0), b=None) == 0 and sim.hbm_bytes() == before
    assert call(sim) == 0 and sim.hbm_bytes() == before + 64 * 24 + 16 * 4      # (the two boxes touch four tiles, one of them both)
    f, b = sim.forcing()
    assert f.tobytes() == good.tobytes() and b.tobytes() == gb.tobytes()      # euler_get_forcing returns what was set
    one = np.zeros((), ea.FORCING_DTYPE)
    assert L.euler_get_forcing(sim.h, one.ctypes.data, None, 0) == 0 and one.tobytes() == good.tobytes()
    assert L.euler_get_forcing(sim.h, one.ctypes.data, gb.ctypes.data, 1) == EULER_EINVAL and L.euler_get_forcing(sim.h, None, None, 0) == EULER_EINVAL
    whole = np.zeros(1, ea.FORCE_BOX_DTYPE)
    whole[0] = (1, 1, X - 2, Y - 2, 1.0, 0.0)
    assert call(sim, f=bad(nboxes=1), b=whole) == 0 and sim.hbm_bytes() == before + 64 * 24 + 16 * 15      # grown
    assert call(sim) == 0 and sim.hbm_bytes() == before + 64 * 24 + 16 * 15                                 # kept
    assert call(sim, f=bad(gx=np.nan)) == EULER_EINVAL and sim.hbm_bytes() == before + 64 * 24 + 16 * 15 and sim.forcing()[0].tobytes() == good.tobytes()
    with pytest.raises(ea.EulerError) as e:
        sim.set_forcing(boxes=[((1, 1, X - 1, 5), (1, 1))])
    assert e.value.code == EULER_EINVAL and "box 0" in str(e.value)
    # the clock: += dt behind every substep, not behind a stage; set_time; a load puts it back to 0 and keeps the forcing
    sim.step()
    t1 = sim.time
    assert abs(t1 - 0.1) < 1e-6
    sim.stage(ea.STAGE_ADVECT_MARKERS, 0.01)
    assert sim.time == t1
    dt = sim.timestep(0.1)
    sim.substep(dt)
    assert sim.time == t1 + float(np.float32(dt))
    sim.time = 7.25
    assert sim.time == 7.25
    for t in (np.nan, np.inf, -np.inf):
        assert L.euler_set_time(sim.h, float(t)) == EULER_EINVAL and sim.time == 7.25
    assert L.euler_set_time(None, 0.0) == EULER_EINVAL and L.euler_get_time(sim.h, None) == EULER_EINVAL
    snap = str(tmp_path / "state.snap")
    sim.save_state(snap)
    sim.load_state(snap)
    assert sim.time == 0.0 and sim.forcing()[0].tobytes() == good.tobytes() and sim.forcing()[1].tobytes() == gb.tobytes()
    sim.time = 3.0
    sim.load_text(scenarios.dam_break(), upscale=True)
    assert sim.time == 0.0 and sim.forcing()[0].tobytes() == good.tobytes()
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    assert call(slab, f=bad(reserved=1)) == EULER_ESTATE and b"slab" in L.euler_last_error()      # 2: in front of "nothing loaded" and of the record
    with pytest.raises(ea.EulerError) as e:
        slab.set_forcing((0, -5))
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()


# ----------------------------------------------------------------------------- the front end
CLI_BOXES = [((10, 3, 30, 12), (4.0, -1.5)), ((20, 8, 40, 16), (-2.25, 3.0)), ((60, 20, 70, 38), (0.5, 0.25))]
CLI_GAUGES = [(ea.GAUGE_LEVEL, (2, 1, 4, 38)), (ea.GAUGE_LEVEL, (95, 1, 97, 38)), (ea.GAUGE_FLUX, (20, 3, 20, 12)), (ea.GAUGE_FLUX, (1, 1, 98, 38))]
CLI_SHAKE_DEG = 30.0


def _cli_flags():
    out = ["--gravity", "%g,%g" % GRAVITY, "--shake", "%g,%g:%g:%g" % (SHAKE[0], SHAKE[1], SHAKE[2], CLI_SHAKE_DEG)]
    for box, force in CLI_BOXES:
        out += ["--force", "%g,%g:%d,%d,%d,%d" % (tuple(force) + tuple(box))]
    return out


def _gauge_flags():
    out = []
    for kind, box in CLI_GAUGES:
        out += ["--gauge", "%s:%d,%d,%d,%d" % ((gref.KINDS[kind],) + tuple(box))]
    return out


def test_cli_forcing(am, tmp_path):
    X, Y = 100, 40
    text = scenarios.dam_break()
    scn = tmp_path / "dam.txt"
    scn.write_text(text)
    base = [EXE, "--dump", "--window", "98x38", "--size", "%dx%d" % (X, Y), "--upscale"]

    def run(*flags, frames=30):
        r = subprocess.run(base + ["--frames", str(frames)] + list(flags) + [str(scn)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    # 30 forced frames with gauges: the frames and the file are the Python composition's, frame for frame
    f = fref.forcing(GRAVITY, SHAKE[:3] + (CLI_SHAKE_DEG * (math.pi / 180.0),))
    o = Oracle(X, Y).load_text(text, upscale=True)
    clock = fref.Clock()
    want_frames, want_csv = [], [gref.CSV_HEADER]
    for k in range(31):
        if k:
            fref.step(am, o, f, CLI_BOXES, clock, acc_at=acc_at)
        want_frames.append(o.render(98, 38))
        recs = gref.gauges_ref(np.array(o.solid), np.array(o.count), np.array(o.u), np.array(o.v), None, CLI_GAUGES)
        want_csv += [gref.csv_line(k, j, kind, recs[j]) for j, (kind, _) in enumerate(CLI_GAUGES)]
    out = tmp_path / "g.csv"
    got = dumped_frames(run(*_cli_flags(), *_gauge_flags(), "--gauges", str(out)))
    assert got == want_frames and out.read_text() == "".join(want_csv)
    assert len(set(want_frames)) > 20
    o.close()
    # with the other modes: the forced run goes through, and differs from the unforced one
    for extra in (["--fit", "--stats", str(tmp_path / "s.csv"), "--ppm", str(tmp_path / "p_"), "--ppm-every", "5", "--edit", "3:solid:40,2,42,20"],
                  ["--view", "5,3,60,30", "--maccormack", "--advection", "rk2"]):
        assert run(*_cli_flags(), *extra, frames=6) != run(*extra, frames=6), extra
    # a run without the flags is byte for byte what it was: the frames of euler_render of a handle that never heard of the forcing
    sim = ea.Simulation(X, Y).load_text(text, upscale=True)
    plain = []
    for k in range(4):
        if k:
            sim.step()
        plain.append(sim.draw(98, 38))
    sim.close()
    assert dumped_frames(run(frames=3)) == plain
    # usage errors: status 1, nothing on stdout
    many = []
    for k in range(65):
        many += ["--force", "1,0:1,1,%d,5" % (k + 1)]
    for bad in (["--gravity", "1"], ["--gravity", "1,2x"], ["--gravity", "nan,0"], ["--gravity", "1e5,0"], ["--shake", "1,2"], ["--shake", "1,2:-1"], ["--shake", "1,2:1:x"],
                ["--shake", "2e4,0:1"], ["--force", "1,2:1,1,5"], ["--force", "1,2:1,1,5,5x"], ["--force", "1,2:0,1,5,5"], ["--force", "1,2:1,1,%d,5" % (X - 1)],
                ["--force", "1,2:6,1,5,5"], ["--force", "1e5,0:1,1,5,5"], many):
        r = subprocess.run(base + ["--frames", "2"] + bad + [str(scn)], capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--gravity GX,GY" in r.stderr and not r.stdout, bad
    assert run(*many[:128], frames=2)      # 64 are taken
