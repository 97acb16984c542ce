"""euler_set_heat on the GPU (docs/heat.md): the temperature against the test-side restatement (tests/heat_ref.py, pinned on the CPU by test_heat_host.py), bit
for bit in the parity mode (every grid here has fewer than 65 536 cells, so `project` is the oracle's): the two stages teacher-forced under each transport,
with viscosity, with a forcing and seven heat boxes, with stirred markers and on the waterfall; free runs; the two "changes no bit" properties against an
untouched handle; the lean forms against the full ones; steps behind an edit; off and on, loads, the field calls and every refusal in order; the known
answers of the host test on the device; the raster byte for byte against numpy, its painter and refusals; the invariant behind edits; the command.  The (ax, ay) of the restatement are euler_forcing_at's own, so no libm difference reaches these tests."""
import ctypes as C

import numpy as np
import pytest

import advect_maccormack_ref as amref
import edit_ref as eref
import euler_amd as ea
import forcing_ref as fref
import heat_ref as href
from euler_amd import scenarios
from observer_util import EULER_EINVAL, EULER_ESTATE, STATE_FIELDS
from oracle_lib import Oracle
from test_gpu_forcing import GRAVITY, LATE_BOX, LATE_START, SHAKE, acc_at, boxes_of, compare_state, dry_box, pair, set_forcing
from test_gpu_parity import assert_bits
from test_heat_host import HEATER, HOT, SIZE, U24, centre_of_heat, closed_tank_text, heater_flux

pytestmark = pytest.mark.gpu

F32 = np.float32
GRIDS = [(100, 40), (103, 41), (264, 136), (1031, 70)]
DYE = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B)
DYE_TMP = (ea.F_DYE_RTMP, ea.F_DYE_GTMP, ea.F_DYE_BTMP)
# (rk2, maccormack, kappa, beta): the four transports, kappa in {0, 0.3, 2.5}, beta in {0, 0.5, -2}
CASES = ((0, 0, 0.0, 0.5), (1, 0, 0.3, -2.0), (0, 1, 2.5, 0.5), (1, 1, 0.3, 0.0), (0, 0, 2.5, -2.0))
AMBIENT = 1.0


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("heat_gpu"))


def heat_boxes_of(Xg, Yg, count):
    """seven boxes: a RATE, a FIX over part of it (FIX behind RATE), the RATE again, one across x = 63 | 64 and y = 63 | 64 (clipped to the interior), one in a
    dry tile, one touching X - 2 and Y - 2, one of a single cell"""
    xi, yi = Xg - 2, Yg - 2
    clip = lambda b: (min(b[0], xi), min(b[1], yi), min(b[2], xi), min(b[3], yi))
    return [(href.RATE, 30.0, (10, 3, 30, 12)), (href.FIX, 4.0, (20, 8, 40, 16)), (href.RATE, 30.0, (10, 3, 30, 12)), (href.RATE, -12.5, clip((60, 60, 70, 70))),
            (href.FIX, 7.0, dry_box(count)), (href.RATE, 5.0, (xi - 4, yi - 3, xi, yi)), (href.FIX, -3.0, (5, 6, 5, 6))]


def set_heat(sim, h, boxes=()):
    sim.set_heat(h["ambient"], h["beta"], h["kappa"], h["source_t"], list(boxes))


def stripes(count, ambient):
    """a field with something to move in every fluid cell, some of them at ambient itself; dry cells at ambient"""
    ys, xs = np.indices(count.shape)
    T = (F32(ambient) + ((xs * 3 + ys * 5) % 9).astype(F32) * F32(0.75) - F32(2.25)).astype(F32)
    T[count == 0] = F32(ambient)
    return T


# ----------------------------------------------------------------------------- the two stages, teacher-forced
def _stage_cases(am, size, frame, viscosity=0.0, text=None, stir=False, cases=CASES, source_t=0.0):
    """stir: STAGE_SOURCES alone, with cells that become fluid without a neighbour that was"""
    sim, o = pair(size, text=text, rainbow=True, viscosity=viscosity)
    for _ in range(frame):
        sim.step(); o.step()
    h = href.heat(AMBIENT, 0.5, 0.0, source_t)
    set_heat(sim, h)
    assert (sim.temperature == F32(AMBIENT)).all()      # switched on: ambient everywhere
    T0 = stripes(np.array(o.count), AMBIENT)
    sim.temperature = T0
    assert_bits(sim.temperature, T0, "the field as set")
    if stir:      # markers dropped into the air far from the water: cells that become fluid with no neighbour that was
        c = np.array(o.count)
        far = [(x, y) for y in range(3, size[1] - 3, 4) for x in range(3, size[0] - 3, 5) if not c[y - 2:y + 3, x - 2:x + 3].any() and not np.array(o.solid)[y - 1:y + 2, x - 1:x + 2].any()][:40]
        assert len(far) > 5
        m = np.concatenate([o.markers.copy(), np.array([(x + 0.5, y + 0.5) for x, y in far], F32)])
        o.set_markers(m); sim.set_markers(m)
    dt = sim.timestep(0.1)
    assert dt == o.timestep(0.1)
    lib = o.lib
    # the front half, STAGE_SOURCES with the heat's extension and source cells
    sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
    lib.eo_advect_markers(o.ptr, C.c_float(dt))
    sim.stage(ea.STAGE_REFRESH_COUNTS)
    lib.eo_refresh_marker_counts(o.ptr)
    sim.stage(ea.STAGE_SOURCES)
    for q in (o.cr, o.cg, o.cb):
        lib.eo_extrapolate(o.ptr, o.f32p(q), 0)
    lib.eo_update_fluid_sources(o.ptr)
    T = T0.copy()
    lonely = href.extend(o, T, h)
    assert_bits(sim.temperature, T, "T behind STAGE_SOURCES")
    new = (np.array(o.prev_count) == 0) & (np.array(o.count) != 0)
    assert new.any() or frame == 0
    if stir:      # (such a cell's velocities are the reference's own 0 / 0 from here on: the stage that makes them is this one, and it is compared above)
        assert lonely > 5 and (T[new] == F32(AMBIENT)).sum() >= lonely
        sim.close(); o.close()
        return
    if source_t:
        assert (np.array(o.source) != 0).any() and (T[np.array(o.source) != 0] == F32(source_t)).all()
    sim.stage(ea.STAGE_EXTRAPOLATE)
    for q, t in ((o.u, 1), (o.v, 2)):
        lib.eo_extrapolate(o.ptr, o.f32p(q), t)
    for q, t in ((o.u, 1), (o.v, 2)):
        lib.eo_zero_bounds(o.ptr, o.f32p(q), t)
    assert_bits(sim.get(ea.F_U), o.u, "u in front of the advection")
    assert_bits(sim.get(ea.F_COUNT), o.count, "count in front of the advection")
    # STAGE_ADVECT_VELOCITY from the same state under every case
    f = fref.forcing(GRAVITY, SHAKE)
    count = np.array(o.count)
    fboxes, hboxes = boxes_of(*size, count), heat_boxes_of(*size, count)
    names = ("u", "v", "utmp", "vtmp", "cr", "cg", "cb", "crtmp", "cgtmp", "cbtmp")
    fields = (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP) + DYE + DYE_TMP
    for n, fld in zip(names[4:], fields[4:]):      # (the tmp fields of the dye hold what the device left there)
        getattr(o, n)[...] = sim.get(fld)
    keep = {n: np.array(getattr(o, n)) for n in names}
    Tk = np.where(count != 0, T, F32(AMBIENT)).astype(F32)      # (the setter writes ambient over the dry cells; no pass reads them)
    moved = 0
    for k, (rk2, mc, kappa, beta) in enumerate(cases):
        sim.set_option(ea.OPT_ADVECT_RK2, rk2)
        sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
        for n, fld in zip(names, fields):
            getattr(o, n)[...] = keep[n]
            sim.set(fld, keep[n])
        hk = href.heat(AMBIENT, beta, kappa, source_t)
        set_heat(sim, hk, hboxes)
        sim.temperature = Tk
        Tr = Tk.copy()
        forced = k % 2 == 0      # every other case under the reference's gravity: ax == 0
        set_forcing(sim, f if forced else fref.DEFAULT, fboxes if forced else [])
        t = (0.0, 0.37, 12.5)[k % 3]
        sim.time = t
        sim.stage(ea.STAGE_ADVECT_VELOCITY, dt)
        if forced:
            href.advect_velocity_stage(am, o, Tr, hk, hboxes, dt, f, fboxes, t, rk2, mc, acc=acc_at(f, t))
        else:
            href.advect_velocity_stage(am, o, Tr, hk, hboxes, dt, None, (), t, rk2, mc)
        what = "%dx%d frame %d rk2=%d mc=%d nu=%g kappa=%g beta=%g" % (size + (frame, rk2, mc, viscosity, kappa, beta))
        assert_bits(sim.temperature, Tr, what + " T")
        for fld, q, n in ((ea.F_UTMP, o.utmp, "utmp"), (ea.F_VTMP, o.vtmp, "vtmp")):
            assert_bits(sim.get(fld), q, what + " " + n)
        if viscosity > 0:      # (the extension's scratch; without it u, v are the stage's input, untouched)
            assert_bits(sim.get(ea.F_U)[:, :-1], o.u[:, :-1], what + " u")
            assert_bits(sim.get(ea.F_V)[:-1, :], o.v[:-1, :], what + " v")
        else:
            assert_bits(sim.get(ea.F_U), keep["u"], what + " u")
            assert_bits(sim.get(ea.F_V), keep["v"], what + " v")
        for fld, q in zip(DYE, (o.cr, o.cg, o.cb)):
            assert_bits(sim.get(fld), q, "%s dye %d" % (what, fld))
        assert (Tr[count == 0] == F32(AMBIENT)).all()
        moved += int((Tr != Tk).sum())
    assert moved > 0
    sim.close(); o.close()


@pytest.mark.parametrize("frame", [0, 6])
@pytest.mark.parametrize("size", GRIDS)
def test_stages_teacher_forced(am, size, frame):
    _stage_cases(am, size, frame)


def test_stages_teacher_forced_with_viscosity(am):
    _stage_cases(am, (264, 136), 6, viscosity=0.5, cases=CASES[1:4])


@pytest.mark.parametrize("size", [(103, 41), (264, 136)])
def test_stages_teacher_forced_with_stirred_markers(am, size):
    _stage_cases(am, size, 6, stir=True)


def test_stages_teacher_forced_on_the_waterfall(am):
    _stage_cases(am, (100, 40), 6, text=scenarios.waterfall(), cases=CASES[1:4], source_t=-6.5)


# ----------------------------------------------------------------------------- free runs
def _free_run(am, size, frames, h, rk2=0, mc=0, forced=True, text=None, edits=(), **kw):
    sim, o = pair(size, text=text, **kw)
    sim.set_option(ea.OPT_ADVECT_RK2, rk2)
    sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
    count = np.array(o.count)
    f = fref.forcing(GRAVITY, SHAKE) if forced else None
    fboxes = boxes_of(*size, count) if forced else []
    hboxes = heat_boxes_of(*size, count)
    if forced:
        set_forcing(sim, f, fboxes)
    set_heat(sim, h, hboxes)
    T = stripes(count, h["ambient"])
    sim.temperature = T
    clock = fref.Clock()
    for k in range(frames):
        for at, op, box in edits:
            if at == k:
                count = np.array(o.count)
                sim.edit_box(op, box)
                edit_oracle(o, op, box)
                compare_state(o, sim, "behind the edit %d" % op)
                if op == ea.EDIT_FILL:      # filled water is at ambient
                    x0, y0, x1, y1 = box
                    new = (np.array(o.count) != 0) & (count == 0)
                    assert new[y0:y1 + 1, x0:x1 + 1].any() and (sim.temperature[new] == F32(h["ambient"])).all()
        sim.step()
        n, it = href.step(am, o, T, h, hboxes, f, fboxes, clock, rk2, mc, acc_at)
        st = sim.stats()
        assert (st.last_substeps, st.last_pcg_iterations) == (n, it), (size, k)
        what = "%dx%d frame %d" % (size + (k,))
        compare_state(o, sim, what)
        assert_bits(sim.temperature, T, what + " T")
        assert st.rng_state == o.c.rng_state and sim.time == clock.t
    assert max(np.abs(o.u).max(), np.abs(o.v).max()) > 1 and len(np.unique(T)) > (1 if text else 50)      # (the waterfall's water all comes from the tap: source_t)
    sim.close(); o.close()


def edit_oracle(o, op, box):
    """euler_edit_box on the oracle's state, by tests/edit_ref.py's restatement"""
    st = eref.edit_state(dict(u=np.array(o.u), solid=np.array(o.solid), source=np.array(o.source), sink=np.array(o.sink), count=np.array(o.count),
                              markers=o.markers.copy(), rng_state=int(o.c.rng_state)), op, box)
    for n in ("solid", "source", "sink", "count"):
        getattr(o, n)[...] = st[n]
    o.set_markers(st["markers"])
    o.c.rng_state = int(st["rng_state"])


@pytest.mark.parametrize("size,forced", [((100, 40), True), ((264, 136), False)])
def test_free_run_against_the_composition(am, size, forced):
    _free_run(am, size, 20, href.heat(AMBIENT, 0.5, 0.3), forced=forced)


def test_free_run_with_maccormack_and_rk2(am):
    _free_run(am, (100, 40), 8, href.heat(0.0, -2.0, 2.5), rk2=1, mc=1)


def test_free_run_on_the_waterfall_with_a_hot_tap(am):
    _free_run(am, (100, 40), 12, href.heat(AMBIENT, 0.5, 0.3, 9.0), forced=False, text=scenarios.waterfall())


def test_steps_behind_edits(am):
    """a wall through the heated water, a notch cleared in it, a block of water filled into the air: the steps behind them match, filled water is at ambient"""
    _free_run(am, (103, 41), 10, href.heat(AMBIENT, 0.5, 0.3), forced=False,
              edits=((3, ea.EDIT_SOLID, (18, 2, 24, 20)), (5, ea.EDIT_CLEAR, (18, 4, 24, 6)), (6, ea.EDIT_FILL, (70, 25, 85, 33))))


# ----------------------------------------------------------------------------- the two properties that change no bit
def _no_bit(options=(), uniform=False, size=(100, 40), frames=10, **kw):
    def make():
        s = ea.Simulation(*size, rainbow=True, **kw)
        for k, v in options:
            s.set_option(k, v)
        return s.load_text(scenarios.dam_break(), upscale=True)

    a, b = make(), make()
    count = b.get(ea.F_COUNT)
    if uniform:      # any beta over a field that is ambient everywhere (1.0: a constant the interpolation's weights reproduce exactly, docs/heat.md)
        b.set_heat(1.0, 3.0, 0.3, 1.0, [(href.FIX, 1.0, (5, 2, 60, 30)), (href.RATE, 0.0, (1, 1, size[0] - 2, size[1] - 2))])
    else:            # beta == 0: a passive scalar
        b.set_heat(AMBIENT, 0.0, 0.3, 2.0, heat_boxes_of(*size, count))
        b.temperature = stripes(count, AMBIENT)
    for k in range(frames):
        a.step(); b.step()
        for fld in STATE_FIELDS + DYE:
            assert_bits(b.get(fld), a.get(fld), "frame %d field %d" % (k, fld))
    sa, sb = a.stats(), b.stats()
    assert (sa.total_substeps, sa.total_pcg_iterations, sa.n_markers, sa.rng_state) == (sb.total_substeps, sb.total_pcg_iterations, sb.n_markers, sb.rng_state)
    T = b.temperature
    if uniform:
        assert (T == F32(1.0)).all()
    else:
        assert len(np.unique(T)) > 50 and (T[b.get(ea.F_COUNT) == 0] == F32(AMBIENT)).all()
    a.close(); b.close()


@pytest.mark.parametrize("uniform", [False, True])
def test_no_bit_changes(uniform):
    _no_bit(uniform=uniform, dot_mode=ea.DOT_SEQUENTIAL)


@pytest.mark.parametrize("uniform", [False, True])
def test_no_bit_changes_with_maccormack_and_rk2(uniform):
    _no_bit(options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)), uniform=uniform, dot_mode=ea.DOT_SEQUENTIAL)


@pytest.mark.parametrize("uniform", [False, True])
def test_no_bit_changes_in_the_tile_local_mode(uniform):
    _no_bit(uniform=uniform, size=(264, 136), dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE)


# ----------------------------------------------------------------------------- the lean forms
def _device_run(size, start, frames, h, hboxes, options=()):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50).load_text(scenarios.dam_break(), upscale=True)
    for key, val in options:
        sim.set_option(key, val)
    for _ in range(start):
        sim.step()
    c0 = sim.get(ea.F_COUNT)
    set_heat(sim, h, hboxes)
    sim.temperature = stripes(c0, h["ambient"])
    out = []
    for _ in range(frames):
        sim.step()
        out.append([sim.get(fld) for fld in STATE_FIELDS] + [sim.temperature])
    sim.close()
    return c0, out


def test_lean_forms_give_the_bits_of_the_full_ones():
    """over a run in which a tile gets wet (test_gpu_forcing.py's LATE_BOX tile) and another dries (asserted), with a heat box in the tile that gets wet"""
    size = (264, 136)
    (x0, y0, x1, y1), _ = LATE_BOX
    tile = (slice(y0 // 64 * 64, y0 // 64 * 64 + 64), slice(x0 // 64 * 64, x0 // 64 * 64 + 64))
    h = href.heat(AMBIENT, 0.5, 0.3)
    hboxes = heat_boxes_of(*size, np.zeros((size[1], size[0]), np.uint8))[:6] + [(href.FIX, 6.0, LATE_BOX[0])]
    c0, lean = _device_run(size, LATE_START, 20, h, hboxes)
    ci = STATE_FIELDS.index(ea.F_COUNT)
    assert not c0[tile].any() and lean[9][ci][tile].any()      # dry at the run's frame 0, wet by its frame 10
    wet0 = [c0[ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64].any() for ty in range(3) for tx in range(5)]
    wet1 = [lean[19][ci][ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64].any() for ty in range(3) for tx in range(5)]
    assert any(a and not b for a, b in zip(wet0, wet1))      # a tile dried
    assert (lean[19][-1][y0:y1 + 1, x0:x1 + 1] == F32(6.0)).any()      # the box has water to heat
    c1, full = _device_run(size, LATE_START, 20, h, hboxes, options=((ea.OPT_NO_TILE_MAP, 1), (ea.OPT_VELOCITY_TWO_PASS, 1), (ea.OPT_MARKERS_TWO_PASS, 1), (ea.OPT_BUILD_TWO_PASS, 1)))
    assert_bits(c1, c0, "count at the start")
    for k, (a, b) in enumerate(zip(lean, full)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert_bits(x, y, "frame %d field %d" % (k, j))


# ----------------------------------------------------------------------------- the surface
def test_off_and_on_loads_and_the_field_calls(tmp_path):
    X, Y = 103, 41
    sim = ea.Simulation(X, Y).load_text(scenarios.dam_break(), upscale=True)
    ref = ea.Simulation(X, Y).load_text(scenarios.dam_break(), upscale=True)
    before = sim.hbm_bytes()
    with pytest.raises(ea.EulerError) as e:
        sim.heat()
    assert e.value.code == EULER_ESTATE
    with pytest.raises(ea.EulerError) as e:
        sim.temperature
    assert e.value.code == EULER_ESTATE
    hboxes = [(href.RATE, 30.0, (10, 3, 30, 12)), (href.FIX, 4.0, (60, 8, 70, 16))]
    sim.set_heat(2.0, 0.5, 0.3, 1.5, hboxes)
    assert sim.hbm_bytes() == before + 2 * X * Y * 4 + 64 * 24 + 16 * 2      # the field and its scratch copy; 64 boxes of 24 bytes, 16 per touched tile
    rec, b = sim.heat()
    assert (rec["ambient"], rec["beta"], rec["kappa"], rec["source_t"], rec["nboxes"]) == (2.0, 0.5, F32(0.3), 1.5, 2)
    assert [(int(k), float(v), (int(a), int(bb), int(c), int(d))) for a, bb, c, d, v, k in b.tolist()] == hboxes
    assert (sim.temperature == F32(2.0)).all()
    count = sim.get(ea.F_COUNT)
    # set_field writes ambient over the dry cells; get_field returns what is there; fill sets the cells of the box that hold markers
    rng = np.random.default_rng(5)
    T = rng.standard_normal((Y, X)).astype(F32) * 50
    sim.temperature = T
    want = np.where(count != 0, T, F32(2.0)).astype(F32)
    assert_bits(sim.temperature, want, "set_field")
    box = (30, 5, 70, 30)
    assert count[5:31, 30:71].any() and not count[5:31, 30:71].all()
    sim.heat_fill(box, -7.5)
    want[5:31, 30:71][count[5:31, 30:71] != 0] = F32(-7.5)
    assert_bits(sim.temperature, want, "heat_fill")
    sim.heat_fill((X - 2, Y - 2, X - 2, Y - 2), 3.0).heat_fill((1, 1, X - 2, Y - 2), 8.0)      # the last cell (dry); the whole interior
    want[count != 0] = F32(8.0)
    assert_bits(sim.temperature, want, "heat_fill over the interior")
    # a later call keeps the field and replaces the rest; off: the handle runs as one that never had heat; on again: ambient everywhere
    sim.set_heat(2.0, -1.0, 0.0, 0.0)
    assert_bits(sim.temperature, want, "the field behind a second euler_set_heat")
    assert sim.heat()[0]["beta"] == -1.0 and len(sim.heat()[1]) == 0
    grown = sim.hbm_bytes()
    sim.heat_off()
    assert sim.hbm_bytes() == grown
    for k in range(5):
        sim.step(); ref.step()
    for fld in STATE_FIELDS:
        assert_bits(sim.get(fld), ref.get(fld), "heat off: field %d" % fld)
    grown = sim.hbm_bytes()      # (the first solves reserved the solver's own ring)
    sim.set_heat(-3.0, 0.5, 0.3)     # (another ambient is fine now: the field starts afresh)
    assert (sim.temperature == F32(-3.0)).all() and sim.hbm_bytes() == grown
    # a load and euler_load_state keep the record and reset the field
    sim.heat_fill((1, 1, X - 2, Y - 2), 4.0)
    for k in range(2):
        sim.step()
    assert (sim.temperature != F32(-3.0)).any()
    snap = str(tmp_path / "state.snap")
    sim.save_state(snap)
    sim.load_state(snap)
    assert (sim.temperature == F32(-3.0)).all() and sim.heat()[0]["kappa"] == F32(0.3)
    sim.heat_fill((1, 1, X - 2, Y - 2), 4.0)
    sim.load_text(scenarios.dam_break(), upscale=True)
    assert (sim.temperature == F32(-3.0)).all() and sim.heat()[0]["beta"] == 0.5
    sim.step()
    sim.close(); ref.close()


def test_refusals_in_order():
    X, Y = 264, 136
    sim = ea.Simulation(X, Y)
    L = sim.L
    good = ea.heat_default()
    good["ambient"], good["beta"], good["kappa"], good["source_t"], good["nboxes"] = 1.0, 0.5, 0.3, 2.0, 2
    gb = np.zeros(2, ea.HEAT_BOX_DTYPE)
    gb[0], gb[1] = (10, 3, 30, 12, 4.0, ea.HEAT_RATE), (60, 60, 70, 70, 0.5, ea.HEAT_FIX)

    def call(s, h=good, b=gb):
        return L.euler_set_heat(s.h if s else None, h.ctypes.data if h is not None else None, b.ctypes.data if b is not None else None)

    def bad(**kw):
        h = good.copy()
        for k, v in kw.items():
            h[k] = v
        return h

    err = L.euler_last_error
    assert call(None) == EULER_EINVAL                                                                  # 1: a null sim
    assert call(sim, h=bad(reserved=1, beta=np.nan)) == EULER_ESTATE and call(sim, h=None) == EULER_ESTATE      # 3: nothing loaded, in front of the record
    sim.load_text(scenarios.dam_break(), upscale=True)
    before = sim.hbm_bytes()
    state = [sim.get(fld) for fld in STATE_FIELDS]
    buf = np.zeros((Y, X), F32)
    # the field calls while heat is off
    assert L.euler_heat_get_field(sim.h, buf.ctypes.data, buf.nbytes) == EULER_ESTATE and L.euler_heat_set_field(sim.h, buf.ctypes.data, buf.nbytes) == EULER_ESTATE
    one, two = good.copy(), gb.copy()
    assert L.euler_heat_fill(sim.h, 1, 1, 2, 2, 1.0) == EULER_ESTATE and L.euler_get_heat(sim.h, one.ctypes.data, None, 0) == EULER_ESTATE

    def order(live):
        out = [(bad(reserved=1, beta=np.nan, kappa=3, nboxes=99), b"reserved"), (bad(reserved2=0.5, ambient=np.inf), b"reserved"),          # 4
               (bad(beta=np.nan, kappa=3, nboxes=99), b"beta"), (bad(ambient=-10000.5), b"ambient"), (bad(source_t=np.inf), b"source_t"), (bad(kappa=np.nan), b"kappa"),      # 5
               (bad(kappa=-1e-3, nboxes=99), b"outside"), (bad(kappa=2.5000002), b"outside")]                                               # 6
        if live:
            out += [(bad(ambient=1.5, nboxes=99), b"live"), (bad(ambient=0.0), b"live")]                                                    # 7
        return out + [(bad(nboxes=-1), b"boxes"), (bad(nboxes=65), b"boxes")]                                                               # 8

    def refusals(live):
        for h, word in order(live):
            assert call(sim, h=h) == EULER_EINVAL and word in err(), (h, err())
        assert call(sim, b=None) == EULER_EINVAL and b"null" in err()
        for at in (0, 1):                                                                                                                  # 9
            for field, val, word in (("kind", 2, "kind"), ("kind", -1, "kind"), ("value", np.nan, "value"), ("value", -1.5e4, "value"), ("x0", 0, "["), ("y0", 0, "["),
                                     ("x1", X - 1, "["), ("y1", Y - 1, "["), ("x0", 80, "["), ("y0", 90, "[")):
                wb = gb.copy()
                wb[field][at] = val
                assert call(sim, b=wb) == EULER_EINVAL and ("box %d: %s" % (at, word)).encode() in err(), (at, field, err())
        wb = gb.copy()
        wb["x0"][0], wb["value"][1] = 0, np.nan
        assert call(sim, b=wb) == EULER_EINVAL and b"box 0: [" in err()      # the first box refused is the one named

    refusals(False)
    assert sim.hbm_bytes() == before      # a refused call changes and allocates nothing
    assert L.euler_get_heat(sim.h, one.ctypes.data, None, 0) == EULER_ESTATE
    for fld, a in zip(STATE_FIELDS, state):
        assert_bits(sim.get(fld), a, "field %d" % fld)
    assert call(sim) == 0
    on = sim.hbm_bytes()
    assert on == before + 2 * X * Y * 4 + 64 * 24 + 16 * 4      # (the two boxes touch four tiles, one of them both)
    T = stripes(sim.get(ea.F_COUNT), 1.0)
    sim.temperature = T
    refusals(True)
    assert sim.hbm_bytes() == on and sim.heat()[0].tobytes() == good.tobytes() and sim.heat()[1].tobytes() == gb.tobytes()
    assert_bits(sim.temperature, T, "the field behind the refused calls")
    assert L.euler_get_heat(sim.h, one.ctypes.data, two.ctypes.data, 1) == EULER_EINVAL and L.euler_get_heat(sim.h, None, None, 0) == EULER_EINVAL
    # the field calls: a null argument, a wrong byte count, a box outside the interior, a value out of range
    for fn in (L.euler_heat_get_field, L.euler_heat_set_field):
        assert fn(None, buf.ctypes.data, buf.nbytes) == EULER_EINVAL and fn(sim.h, None, buf.nbytes) == EULER_EINVAL
        assert fn(sim.h, buf.ctypes.data, buf.nbytes - 4) == EULER_EINVAL and fn(sim.h, buf.ctypes.data, buf.nbytes + 4) == EULER_EINVAL
    for v in (np.nan, np.inf, -np.inf, 10000.5, -2e4):
        w = T.copy()
        w[Y // 2, X // 2] = v
        assert L.euler_heat_set_field(sim.h, w.ctypes.data, w.nbytes) == EULER_EINVAL and b"cell" in err()
        assert L.euler_heat_fill(sim.h, 1, 1, 5, 5, float(v)) == EULER_EINVAL and b"value" in err()
    assert L.euler_heat_fill(None, 1, 1, 5, 5, 1.0) == EULER_EINVAL
    for box in ((0, 1, 5, 5), (1, 0, 5, 5), (1, 1, X - 1, 5), (1, 1, 5, Y - 1), (6, 1, 5, 5), (1, 6, 5, 5)):
        assert L.euler_heat_fill(sim.h, *box, 1.0) == EULER_EINVAL and b"interior" in err()
    assert_bits(sim.temperature, T, "the field behind the refused field calls")
    assert sim.hbm_bytes() == on
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    assert call(slab, h=bad(reserved=1)) == EULER_ESTATE and b"slab" in err()      # 2: in front of "nothing loaded" and of the record
    assert L.euler_heat_get_field(slab.h, buf.ctypes.data, buf.nbytes) == EULER_ESTATE and b"slab" in err()
    assert L.euler_heat_fill(slab.h, 1, 1, 5, 5, 1.0) == EULER_ESTATE and b"slab" in err()
    with pytest.raises(ea.EulerError) as e:
        slab.set_heat(0.0, 0.5)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()


# ----------------------------------------------------------------------------- the known answers of the host test, on the device
def test_diffusion_conserves_heat_in_a_still_tank():
    """test_heat_host.py's bound: N S u M (32 c + 1) 1.01"""
    sim = ea.Simulation(*SIZE).load_half_tank()
    sim.set_forcing((0, 0))
    sim.set_heat(0.0, 0.0, 2.5)
    sim.heat_fill(HOT, 50.0)
    cn = sim.get(ea.F_COUNT) != 0
    T = sim.temperature
    T[cn] += F32(0.37)
    sim.temperature = T
    N, M, s0 = int(cn.sum()), float(np.abs(T).max()), float(T[cn].astype(np.float64).sum())
    for _ in range(8):
        sim.step()
    assert sim.stats().total_substeps == 8 and not sim.get(ea.F_U).view(np.uint32).any() and not sim.get(ea.F_V).view(np.uint32).any()
    T1 = sim.temperature
    s1 = float(T1[cn].astype(np.float64).sum())
    bound = N * 8 * U24 * M * (32 * 0.25 + 1) * 1.01
    print("sum T %.9g -> %.9g: off by %.3g, bound %.3g" % (s0, s1, abs(s1 - s0), bound))
    assert abs(s1 - s0) <= bound and float(T1.max()) < M and int((T1[cn] > 0.371).sum()) > 16 * 8
    sim.close()


def test_maximum_principle():
    """test_heat_host.py's bound: [lo, hi] widened by 32 u A per substep"""
    sim = ea.Simulation(100, 40).load_text(scenarios.dam_break(), upscale=True)
    sim.set_heat(0.0, 0.0, 2.5, -4.0, [(href.FIX, 6.0, (10, 1, 40, 6)), (href.FIX, -2.5, (30, 4, 60, 12))])
    count = sim.get(ea.F_COUNT)
    ys, xs = np.indices(count.shape)
    sim.temperature = np.where(count != 0, F32(-4.0) + ((xs + ys) % 11).astype(F32), F32(0)).astype(F32)
    A = 6.0 * 1.001
    for k in range(20):
        sim.step()
        T, sub = sim.temperature, sim.stats().total_substeps
        w = 32 * U24 * A * sub
        assert -4.0 - w <= float(T.min()) and float(T.max()) <= 6.0 + w, (k, T.min(), T.max(), w)
    assert np.abs(sim.get(ea.F_U)).max() > 1 and sub > 20
    sim.close()


@pytest.mark.parametrize("value,gy", [(5.0, -10.0), (-5.0, -10.0), (5.0, 10.0), (-5.0, 10.0)])
def test_a_hot_blob_rises_and_a_cold_one_sinks(value, gy):
    X, Y = SIZE
    sim = ea.Simulation(X, Y).load_text(closed_tank_text(X, Y))
    sim.set_forcing((0, gy))
    sim.set_heat(20.0, 0.5)
    sim.heat_fill((24, 14, 39, 25), 20.0 + value)

    class View:      # what centre_of_heat reads
        pass
    v = View()
    v.count, v.Y = sim.get(ea.F_COUNT), Y
    y0 = centre_of_heat(v, sim.temperature, 20.0)
    for _ in range(6):
        sim.step()
    v.count = sim.get(ea.F_COUNT)
    y1 = centre_of_heat(v, sim.temperature, 20.0)
    assert (y1 - y0) * value * -gy > 0 and abs(y1 - y0) > 0.05
    sim.close()


def test_a_heater_on_the_floor_drives_an_upward_flux():
    sim = ea.Simulation(*SIZE).load_half_tank()
    sim.set_heat(0.0, 0.5, 0.2, 0.0, [HEATER])
    for _ in range(5):
        sim.step()
    assert heater_flux(sim.get(ea.F_SOLID), sim.get(ea.F_COUNT), sim.get(ea.F_U), sim.get(ea.F_V)) > 0
    sim.close()


# ----------------------------------------------------------------------------- the raster and its painter
def _raster_state(size, frames, ambient=1.0):
    """a device state with water in motion and a field that holds, next to the stripes, cells exactly at ambient (d = +0), just below it, and differences beyond
    qv's clamp on either side.  (A NaN or an infinity cannot be put into T through the interface - euler_heat_set_field refuses them, every pass keeps finite values
    finite -; tests/test_heat_host.py plants them in the restatement.)"""
    sim = ea.Simulation(*size).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(frames):
        sim.step()
    sim.set_heat(ambient, 0.5, 0.3)
    count = sim.get(ea.F_COUNT)
    T = stripes(count, ambient)
    ys, xs = np.nonzero(count)
    for k, v in enumerate((ambient, np.nextafter(F32(ambient), F32(-9)), 1e4, -1e4, ambient + 4096.0, ambient - 4097.0, 3.0e-7 + ambient)):
        T[ys[k * 37 % len(ys)], xs[k * 37 % len(ys)]] = v
    sim.temperature = T
    return sim, sim.temperature


@pytest.mark.parametrize("size,frames", [((103, 41), 8), ((264, 136), 30)])
def test_raster_against_numpy(size, frames):
    X, Y = size
    sim, T = _raster_state(size, frames)
    solid, sink, count = sim.get(ea.F_SOLID), sim.get(ea.F_SINK), sim.get(ea.F_COUNT)
    ys, xs = np.nonzero(count)
    wet = (int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))
    cases = [((1, 1, X - 2, Y - 2), 7, 5), ((1, 1, X - 2, Y - 2), X - 2, 1), ((1, 1, X - 2, Y - 2), 1, Y - 2), ((1, 1, X - 2, Y - 2), 1, 1),      # the whole interior, ragged
             ((3, 2, X - 5, Y - 4), 13, 11), ((5, 3, 70, 33), 66, 31), (wet + wet, 1, 1), ((X - 2, Y - 2, X - 2, Y - 2), 1, 1)]                  # a box of one cell: wet, dry
    if X < 128:
        cases.append(((1, 1, X - 2, Y - 2), X - 2, Y - 2))      # one cell per pixel
    seen = 0
    for box, w, h in cases:
        got = sim.heat_raster(w, h, box)
        want = href.raster(T, solid, sink, count, 1.0, box, w, h)
        assert got.tobytes() == want.tobytes(), (box, w, h)
        ov = sim.overview(w, h, box)
        assert np.array_equal(got["cells"], ov["cells"]) and np.array_equal(got["water"], ov["water"])      # euler_overview_box's box, edges and water
        painted = ea.heat_paint(got, ov, 1.0, 2.5)
        assert np.array_equal(painted["dye"], href.paint(want, 2.5))
        seen += int(got["water"].sum())
    whole = sim.heat_raster(1, 1)[0, 0]
    assert seen > 0 and whole["max_above"] == F32(1e4) - F32(1.0) and whole["max_below"] == F32(1.0) - F32(-1e4) and int(whole["t_pos"]) >= 2 * (4096 << 20) and int(whole["t_neg"]) >= 2 * (4096 << 20)
    # a pass that only reads: the field and the state keep their bits
    assert_bits(sim.temperature, T, "T behind the rasters")
    sim.close()


def test_raster_refusals():
    X, Y = 103, 41
    sim = ea.Simulation(X, Y)
    L = sim.L
    out = np.zeros((3, 4), ea.HEAT_PX_DTYPE)
    call = lambda s, box=(1, 1, 50, 30), w=4, h=3, dst=out, nbytes=None: L.euler_heat_raster(s.h if s else None, *box, w, h, dst.ctypes.data if dst is not None else None, out.nbytes if nbytes is None else nbytes)
    assert call(None) == EULER_EINVAL and call(sim, dst=None) == EULER_EINVAL
    assert call(sim) == EULER_ESTATE                                   # nothing loaded
    sim.load_text(scenarios.dam_break(), upscale=True)
    assert call(sim) == EULER_ESTATE and b"heat is off" in L.euler_last_error()
    sim.set_heat(1.0, 0.5)
    before = sim.hbm_bytes()
    for box in ((0, 1, 50, 30), (1, 0, 50, 30), (1, 1, X - 1, 30), (1, 1, 50, Y - 1), (51, 1, 50, 30), (1, 31, 50, 30)):
        assert call(sim, box=box) == EULER_EINVAL and b"interior" in L.euler_last_error()
    for w, h in ((0, 3), (4, 0), (51, 3), (4, 31), (-1, 3)):
        assert call(sim, w=w, h=h) == EULER_EINVAL and b"raster" in L.euler_last_error()
    assert call(sim, nbytes=out.nbytes - 32) == EULER_EINVAL and call(sim, nbytes=out.nbytes + 32) == EULER_EINVAL and b"bytes" in L.euler_last_error()
    assert sim.hbm_bytes() == before                                   # a refused call allocates nothing
    assert call(sim) == 0 and sim.hbm_bytes() == before + out.nbytes and out["cells"].sum() == 50 * 30
    sim.heat_off()
    assert call(sim) == EULER_ESTATE
    sim.close()
    slab = ea.Simulation(264, 136, slab=(0, 1))
    assert call(slab) == EULER_ESTATE and b"slab" in L.euler_last_error()
    slab.close()


# ----------------------------------------------------------------------------- the invariant between substeps: behind an edit
def test_water_filled_where_an_edit_emptied_starts_at_ambient():
    """DRAIN, SOLID and SINK empty cells; with heat on they take ambient at once, so the field read back holds the invariant and a FILL before any step starts there"""
    X, Y = 103, 41
    sim = ea.Simulation(X, Y).load_text(scenarios.dam_break(), upscale=True)
    sim.set_heat(AMBIENT, 0.5, 0.3)
    sim.heat_fill((1, 1, X - 2, Y - 2), 9.0)
    box = (20, 12, 40, 25)
    sl = (slice(12, 26), slice(20, 41))
    assert sim.get(ea.F_COUNT)[sl].all() and (sim.temperature[sl] == F32(9.0)).all()
    for op in (ea.EDIT_DRAIN, ea.EDIT_SOLID, ea.EDIT_CLEAR):      # (CLEAR takes the wall away again: the cells stay empty)
        sim.edit_box(op, box)
        T, count = sim.temperature, sim.get(ea.F_COUNT)
        assert not count[sl].any() and (T[count == 0] == F32(AMBIENT)).all() and (T[count != 0] == F32(9.0)).all(), op
    sim.edit_box(ea.EDIT_FILL, box)
    T, count = sim.temperature, sim.get(ea.F_COUNT)
    assert count[sl].all() and (T[sl] == F32(AMBIENT)).all() and (T[count == 0] == F32(AMBIENT)).all()
    sim.step()
    T, count = sim.temperature, sim.get(ea.F_COUNT)
    assert (T[count == 0] == F32(AMBIENT)).all() and T.max() <= 9.0 * (1 + 1e-6) and T[count != 0].min() >= AMBIENT * (1 - 1e-6)      # (a few roundings of the interpolation)
    sim.close()


# ----------------------------------------------------------------------------- the front end
CLI_HEAT = href.heat(16.0, 0.5, 0.3)
CLI_HEAT_BOXES = [(href.FIX, 60.0, (10, 1, 40, 3)), (href.RATE, -20.0, (20, 8, 45, 16)), (href.FIX, 60.0, (10, 1, 40, 3))]
CLI_HEAT_INITS = [(40.0, (5, 10, 30, 25)), (-8.0, (25, 15, 50, 28))]


def _cli_heat_flags(h=CLI_HEAT, boxes=CLI_HEAT_BOXES, inits=CLI_HEAT_INITS):
    out = ["--heat", "%g:%g:%g" % (h["ambient"], h["beta"], h["kappa"])]
    for kind, value, box in boxes:
        out += ["--heat-box", "%s:%g:%d,%d,%d,%d" % ((("fix", "rate")[kind], value) + tuple(box))]
    for value, box in inits:
        out += ["--heat-init", "%g:%d,%d,%d,%d" % ((value,) + tuple(box))]
    return out


def test_cli_heat(am, tmp_path):
    import subprocess
    from observer_util import EXE, dumped_frames
    X, Y = 100, 40
    scn = tmp_path / "dam.txt"
    scn.write_text(scenarios.dam_break())
    fall = tmp_path / "fall.txt"
    fall.write_text(scenarios.waterfall())
    base = [EXE, "--dump", "--window", "98x38", "--size", "%dx%d" % (X, Y), "--upscale"]

    def run(*flags, frames=20, scenario=scn):
        r = subprocess.run(base + ["--frames", str(frames)] + list(flags) + [str(scenario)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    def composed(text, h, boxes, inits, frames, f=None, rk2=0, mc=0):
        o = Oracle(X, Y).load_text(text, upscale=True)
        T = href.field(o, h)
        for value, (x0, y0, x1, y1) in inits:      # euler_heat_fill: the cells of the box that hold markers
            sub = T[y0:y1 + 1, x0:x1 + 1]
            sub[np.array(o.count)[y0:y1 + 1, x0:x1 + 1] != 0] = F32(value)
        clock, out = fref.Clock(), []
        for k in range(frames + 1):
            if k:
                href.step(am, o, T, h, boxes, f, (), clock, rk2, mc, acc_at)
            out.append(o.render(98, 38))
        o.close()
        return out

    # the frames are the composition's, frame for frame; and not those of a run without heat
    want = composed(scenarios.dam_break(), CLI_HEAT, CLI_HEAT_BOXES, CLI_HEAT_INITS, 20)
    assert dumped_frames(run(*_cli_heat_flags())) == want and len(set(want)) > 15
    assert dumped_frames(run()) != want
    # ... with --gravity, --maccormack and --advection rk2; and a hot tap on the waterfall
    f = fref.forcing((2.0, -9.0))
    want = composed(scenarios.dam_break(), CLI_HEAT, CLI_HEAT_BOXES, CLI_HEAT_INITS, 8, f, 1, 1)
    assert dumped_frames(run(*_cli_heat_flags(), "--gravity", "2,-9", "--maccormack", "--advection", "rk2", frames=8)) == want
    tap = href.heat(0.0, -2.0, 0.0, 5.0)
    want = composed(scenarios.waterfall(), tap, [], [], 12)
    assert dumped_frames(run("--heat", "0:-2", "--heat-source", "5", frames=12, scenario=fall)) == want
    # with the pictures: --paint heat:S colours --fit, --view and --ppm; the run goes through and differs from the unpainted one
    for extra in (["--fit"], ["--view", "5,3,60,30"], ["--fit", "--edit", "3:solid:40,2,42,20", "--ppm", str(tmp_path / "p_"), "--ppm-every", "3"]):
        assert run(*_cli_heat_flags(), *extra, "--paint", "heat:20", frames=6) != run(*_cli_heat_flags(), *extra, frames=6), extra
    assert (tmp_path / "p_000003.ppm").exists() or len(list(tmp_path.glob("p_*"))) > 0
    # usage errors: status 1, nothing on stdout
    many = ["--heat", "0:1"]
    for k in range(65):
        many += ["--heat-box", "fix:1:1,1,%d,5" % (k + 1)]
    for bad in (["--heat", "1"], ["--heat", "1:2x"], ["--heat", "nan:0"], ["--heat", "1e5:0"], ["--heat", "0:1:2.6"], ["--heat", "0:1:-1"], ["--heat", "0:1", "--heat-source", "x"],
                ["--heat", "0:1", "--heat-source", "1e5"], ["--heat", "0:1", "--heat-box", "fix:1:1,1,5"], ["--heat", "0:1", "--heat-box", "hold:1:1,1,5,5"],
                ["--heat", "0:1", "--heat-box", "fix:1:0,1,5,5"], ["--heat", "0:1", "--heat-box", "rate:1:1,1,%d,5" % (X - 1)], ["--heat", "0:1", "--heat-box", "fix:1:6,1,5,5"],
                ["--heat", "0:1", "--heat-box", "fix:1e5:1,1,5,5"], ["--heat", "0:1", "--heat-init", "1:1,1,5"], ["--heat", "0:1", "--heat-init", "1:1,1,5,%d" % (Y - 1)],
                ["--heat", "0:1", "--heat-init", "nan:1,1,5,5"], ["--heat", "0:1", "--fit", "--paint", "heat:0"], ["--heat", "0:1", "--paint", "heat:5"],
                ["--heat-box", "fix:1:1,1,5,5"], ["--heat-init", "1:1,1,5,5"], ["--heat-source", "3"], ["--fit", "--paint", "heat:5"], many):
        r = subprocess.run(base + ["--frames", "2"] + bad + [str(scn)], capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--heat AMBIENT:BETA" in r.stderr and not r.stdout, bad
    # without --heat every byte is as before: the frames of a handle that never heard of it
    sim = ea.Simulation(X, Y).load_text(scenarios.dam_break(), upscale=True)
    plain = []
    for k in range(4):
        if k:
            sim.step()
        plain.append(sim.draw(98, 38))
    sim.close()
    assert dumped_frames(run(frames=3)) == plain
