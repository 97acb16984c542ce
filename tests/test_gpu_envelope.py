"""The run-long envelopes on the GPU (docs/envelope.md): arrival time, wet time, peak speed squared and peak pressure per cell, gathered at the end of every
substep.  Against the test-side restatement (tests/envelope_ref.py over the CPU oracle, pinned by test_envelope_host.py, which also checks that the scenes here are
not trivial), bit for bit in the parity mode: the hook teacher-forced behind euler_stage(PROJECT), free runs under the three transports, with a forcing, with the
heat and across a SOLID edit.  Against the handle's own history in the tile-local and multilevel modes: the planes equal the fold of the fields a twin handle shows
after every substep.  Then what the feature must not do (leave a trace in the state, launch anything while it is off), the tile map, the store and its refusals, and
the raster against numpy."""
import ctypes as C

import numpy as np
import pytest

import advect_maccormack_ref as amref
import envelope_ref as er
import euler_amd as ea
from observer_util import EULER_EINVAL, EULER_ESTATE, STATE_FIELDS, no_trace_pair
from oracle_lib import Oracle
from test_envelope_host import (EDIT_FRAME, FORCING, FRAMES, HEAT, HEAT_BOXES, SCENES, TRANSPORTS, WALL_BOX, assert_planes, oracle_run, scene)
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu
NAMES = ("solid", "count", "u", "v", "p")
FIELD = {"solid": ea.F_SOLID, "count": ea.F_COUNT, "u": ea.F_U, "v": ea.F_V, "p": ea.F_PRESSURE}
MODES = {      # Simulation keywords of the solver modes the history tests run in
    "tile": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=400, resident=ea.RESIDENT_OFF),
    "resident": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=400),
    "multilevel": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=400),
}


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("envelope_gpu"))


def load(name, **kw):
    size, text, up = scene(name)
    return ea.Simulation(*size, **kw).load_text(text, upscale=up)


def planes(sim):
    """the handle's planes as an envelope_ref.Envelope"""
    ch, n = sim.envelope()
    e = er.Envelope(sim.X, sim.Y, ch)
    e.substeps = n
    for c in e.planes:
        e.planes[c] = sim.envelope_field(c).view(np.uint32)
    return e


def state(sim):
    return [sim.get(FIELD[n]) for n in NAMES]


# ----------------------------------------------------------------------------- against the restatement, parity mode
@pytest.mark.parametrize("name", ["waterfall", "flume", "wide"])
@pytest.mark.parametrize("frame", [3, 9])
def test_hook_behind_a_teacher_forced_project_stage(am, name, frame):
    size, text, up = scene(name)
    sim = load(name)
    o = Oracle(*size).load_text(text, upscale=up)
    for _ in range(frame):
        sim.step(); o.step()
    assert_bits(sim.get(ea.F_U), o.u, "u at frame %d" % frame)
    sim.set_envelope(ea.ENV_ALL)
    env = er.Envelope(*size)
    dt0 = sim.timestep(0.1)
    assert dt0 == o.timestep(0.1)
    for k, (dt, t) in enumerate(((dt0, 0.0), (float(np.float32(dt0 * 0.5)), 0.37), (float(np.float32(dt0 * 0.125)), 12.5))):
        for st in range(ea.STAGE_PROJECT):
            sim.stage(st, dt)
        er.front_half(am, o, dt, t)
        sim.set(ea.F_UTMP, np.array(o.utmp)); sim.set(ea.F_VTMP, np.array(o.vtmp))      # the oracle's own input to the stage
        sim.time = t
        sim.stage(ea.STAGE_PROJECT, dt)
        assert sim.time == t      # a stage is not a substep: the clock stands
        er.project(o, env, dt, t)
        assert_bits(sim.get(ea.F_PRESSURE), o.p, "%s frame %d dt %d: pressure" % (name, frame, k))
        assert_planes(planes(sim), env, "%s frame %d dt %d" % (name, frame, k))
    # a repeated stage call accumulates again with the same t_end (documented): the same system is solved again, the same state is folded once more
    sim.stage(ea.STAGE_PROJECT, dt)
    er.fold(env, o, t, dt)
    assert_planes(planes(sim), env, "%s frame %d: the stage repeated" % (name, frame))
    assert sim.envelope() == (ea.ENV_ALL, 4)
    sim.close(); o.close()


def _free_run(sim, frames=FRAMES, at_frame=None):
    sim.set_envelope(ea.ENV_ALL)
    for f in range(frames):
        if at_frame:
            at_frame(f)
        sim.step()


def _against(sim, r, what):
    assert_bits(sim.get(ea.F_U), r.u, what + ": u behind the run")
    assert sim.time == r.t_final and sim.envelope() == (ea.ENV_ALL, len(r.substeps))
    assert_planes(planes(sim), r.env, what)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("transport", TRANSPORTS)
def test_free_runs_against_the_restatement(am, name, transport):
    rk2, mc = transport
    sim = load(name)
    sim.set_option(ea.OPT_ADVECT_RK2, rk2)
    sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
    _free_run(sim)
    _against(sim, oracle_run(am, name, rk2, mc), "%s rk2=%d mc=%d" % (name, rk2, mc))
    sim.close()


def test_free_run_with_a_forcing(am):
    sim = load("flume")
    f = FORCING
    sim.set_forcing((f["gx"], f["gy"]), (f["shake_x"], f["shake_y"], f["shake_hz"], f["shake_phase"]), [])
    _free_run(sim)
    _against(sim, oracle_run(am, "flume", forced=True), "flume, forced")
    sim.close()


def test_free_run_with_the_heat_on(am):
    sim = load("flume")
    sim.set_heat(HEAT["ambient"], HEAT["beta"], HEAT["kappa"], HEAT["source_t"], list(HEAT_BOXES))
    _free_run(sim)
    _against(sim, oracle_run(am, "flume", heated=True), "flume, heated")
    sim.close()


@pytest.mark.parametrize("name", ["waterfall", "dam"])
def test_solid_edit_over_wet_cells_keeps_their_words(am, name):
    r = oracle_run(am, name, edit=True)
    sim = load(name)
    _free_run(sim, at_frame=lambda f: f == EDIT_FRAME and sim.edit_box(ea.EDIT_SOLID, r.wall))
    _against(sim, r, "%s with a wall raised at frame %d" % (name, EDIT_FRAME))
    x0, y0, x1, y1 = r.wall
    assert sim.get(ea.F_SOLID)[y0:y1 + 1, x0:x1 + 1].all() and (sim.envelope_field(ea.ENV_WET)[y0:y1 + 1, x0:x1 + 1] > 0)[r.wet_before].all()
    sim.close()


# ----------------------------------------------------------------------------- against the handle's own history
@pytest.mark.parametrize("mode", sorted(MODES))
def test_planes_are_the_fold_of_the_substeps_a_twin_shows(mode):
    """twin handles stepped substep by substep; the one without the envelope is read back after every substep and folded on the host"""
    a, b = load("wide", **MODES[mode]), load("wide", **MODES[mode])
    a.set_envelope(ea.ENV_ALL)
    env = er.Envelope(a.X, a.Y)
    gauge_seen = 0.0
    for f in range(FRAMES):
        left, n = np.float32(0.1), 0
        while left > 0 and n < 8:
            dt = a.timestep(float(left))
            assert b.timestep(float(left)) == dt
            t = b.time
            a.substep(dt); b.substep(dt)
            er.update(env, *state(b), t, dt)
            left = np.float32(left - np.float32(dt))
            n += 1
        assert a.time == b.time
        gauge_seen = max(gauge_seen, float(b.gauges([(ea.GAUGE_PRESSURE, WALL_BOX)])[0]["max_a"]))      # what a look per frame sees
    assert_bits(a.get(ea.F_U), b.get(ea.F_U), mode + ": u of the twins")
    got = planes(a)
    assert_planes(got, env, mode)
    x0, y0, x1, y1 = WALL_BOX
    peak = float(got.f(er.PRESSURE)[y0:y1 + 1, x0:x1 + 1].max())
    px = a.envelope_raster(WALL_BOX, 1, 1)[0, 0]
    assert float(np.array(px["p_max"]).view(np.float32)) == peak
    print("%s: peak pressure beside the wall %.6g, the largest a gauge per frame saw %.6g" % (mode, peak, gauge_seen))
    assert peak > gauge_seen > 0      # (test_envelope_host.py: on the oracle the peak falls between two frames, by more than 1 %)
    print("   resident_info", a.resident_info())
    a.close(); b.close()


# ----------------------------------------------------------------------------- no trace
OPTION_SETS = {"parity": ({}, ()), "tile": (MODES["resident"], ()),
               "full forms": ({}, ((ea.OPT_NO_TILE_MAP, 1), (ea.OPT_VELOCITY_TWO_PASS, 1), (ea.OPT_MARKERS_TWO_PASS, 1), (ea.OPT_BUILD_TWO_PASS, 1)))}


@pytest.mark.parametrize("which", sorted(OPTION_SETS))
def test_envelope_leaves_no_trace_in_the_state(which):
    kw, options = OPTION_SETS[which]
    made = []

    def make():      # the first handle without, the second (the one looked at) with every channel on
        s = load("wide", **kw)
        for k, v in options:
            s.set_option(k, v)
        if made:
            s.set_envelope(ea.ENV_ALL)
        made.append(s)
        return s

    def look(s, stepped):
        assert s.envelope()[0] == ea.ENV_ALL
        s.envelope_raster(None, 9, 5)
        s.envelope_field(ea.ENV_PRESSURE)

    a, b = no_trace_pair(make, look, None, STATE_FIELDS, FRAMES, compare_every=5)
    assert a.envelope() == (0, 0) and b.envelope()[1] > FRAMES
    assert (b.envelope_field(ea.ENV_WET) > 0).any()
    a.close(); b.close()


# ----------------------------------------------------------------------------- the tile map and the edges
def test_tile_map_off_gives_the_same_planes_and_dry_tiles_keep_their_words(am):
    r = oracle_run(am, "wide")
    sim = load("wide")
    sim.set_option(ea.OPT_NO_TILE_MAP, 1)
    _free_run(sim)
    _against(sim, r, "wide, NO_TILE_MAP")      # (test_free_runs_against_the_restatement: the same planes with the map)
    got = planes(sim)
    hit = got.planes[er.ARRIVAL] != er.NEVER
    dry = 0
    for ty in range(0, sim.Y, 64):
        for tx in range(0, sim.X, 64):
            t = (slice(ty, ty + 64), slice(tx, tx + 64))
            if not hit[t].any():
                dry += 1
                assert all(not got.planes[c][t].any() for c in (er.WET, er.SPEED, er.PRESSURE))
    assert dry >= 6
    sim.close()


@pytest.mark.parametrize("size", [(100, 40), (103, 41), (264, 136)])
def test_fluid_cells_on_the_interior_edges_are_recorded(size):
    """the whole interior under water: the cells at x = 1, x = X - 2, y = 1 and y = Y - 2 are fluid in the first substep"""
    Xg, Yg = size
    text = "\n".join("0" * (Xg - 2) for _ in range(Yg - 2)) + "\n"
    sim = ea.Simulation(Xg, Yg).load_text(text)
    o = Oracle(Xg, Yg).load_text(text)
    sim.set_envelope(ea.ENV_ALL)
    env = er.Envelope(Xg, Yg)
    dt = sim.timestep(0.1)
    assert dt == o.timestep(0.1)
    sim.substep(dt)
    er.front_half(None, o, dt, 0.0)
    er.project(o, env, dt, 0.0)
    got = planes(sim)
    assert_planes(got, env, "%d x %d full of water" % size)
    hit = got.planes[er.ARRIVAL] != er.NEVER
    for edge in (hit[1:-1, 1], hit[1:-1, Xg - 2], hit[1, 1:-1], hit[Yg - 2, 1:-1]):
        assert edge.any()
    assert not hit[0, :].any() and not hit[-1, :].any() and not hit[:, 0].any() and not hit[:, -1].any()
    sim.close(); o.close()


# ----------------------------------------------------------------------------- launch accounting
def _launches(s):
    return {k: v[1] for k, v in s.profile().items()}


@pytest.mark.parametrize("mode", ["parity", "tile"])
def test_launch_accounting(mode):
    kw = {} if mode == "parity" else MODES["tile"]

    def make():
        s = load("flume", **kw)
        s.profile_enable(ea.profile_class_names())
        return s

    def run(s, frames=3):
        s.step()      # (the first frame settles what a set or a load invalidated)
        s.profile_reset()
        n0 = s.stats().total_substeps
        for _ in range(frames):
            s.step()
        return _launches(s), s.stats().total_substeps - n0

    plain = make()
    base, nsub = run(plain)
    cleared = make()
    cleared.set_envelope(ea.ENV_ALL).set_envelope(0)
    assert run(cleared) == (base, nsub)      # set and cleared: what a handle that called nothing launches, class by class
    for channels, misc in ((ea.ENV_ARRIVAL | ea.ENV_WET, 1), (ea.ENV_SPEED, 1), (ea.ENV_PRESSURE, 1), (ea.ENV_ALL, 2)):
        s = make()
        s.set_envelope(channels)
        got, n = run(s)
        assert n == nsub
        extra = {k: got.get(k, 0) - base.get(k, 0) for k in set(got) | set(base) if got.get(k, 0) != base.get(k, 0)}
        print("%s, channels %d: %d substeps, launches more than without: %r" % (mode, channels, n, extra))
        assert extra.pop("misc") == misc * n      # the cells pass and the pressure pass: one launch each per substep
        if channels & ea.ENV_PRESSURE:      # what eu_pressure_current owes behind a one-pass velocity update: the clamp, and the last p += alpha s where the solve left it
            assert extra.pop("velocity_update") == n and 0 <= extra.pop("update_pr", 0) <= n
        assert not extra
        s.close()
    plain.close(); cleared.close()


# ----------------------------------------------------------------------------- the store
def test_store_bytes_channels_reset_round_trip_and_loads(tmp_path):
    sim = load("flume")
    Xg, Yg = sim.X, sim.Y
    plane = 4 * Xg * Yg
    T = (Xg + 63 + 95) // 96 * 96      # records per band (docs/envelope.md "the store"): X + 63 live ones in whole units of 96, a stride of that in units of 32 plus 64
    p_plane = 4 * ((Yg + 63) // 64) * ((T + 31) // 32 * 32 + 64) * 64      # the pressure's plane lies in the solver's skewed order: 4 bytes per element of a skewed array

    def grows(channels):      # what one call adds to euler_hbm_bytes (stepping may allocate other buffers on first use: each call is measured on its own)
        b0 = sim.hbm_bytes()
        sim.set_envelope(channels)
        return sim.hbm_bytes() - b0

    assert grows(ea.ENV_WET) == plane and sim.envelope() == (ea.ENV_WET, 0)
    for _ in range(4):
        sim.step()
    n4 = sim.envelope()[1]
    wet4 = sim.envelope_field(ea.ENV_WET)
    assert n4 >= 4 and (wet4 > 0).any()
    # enabled later: the others' words stay, the new planes start fresh, the count goes on
    assert grows(ea.ENV_WET | ea.ENV_ARRIVAL | ea.ENV_SPEED) == 2 * plane and sim.envelope() == (7, n4)
    assert_bits(sim.envelope_field(ea.ENV_WET), wet4, "wet behind enabling more channels")
    assert (sim.envelope_field(ea.ENV_ARRIVAL).view(np.uint32) == er.NEVER).all() and not sim.envelope_field(ea.ENV_SPEED).view(np.uint32).any()
    assert grows(ea.ENV_ALL) == p_plane and grows(ea.ENV_ALL) == 0
    sim.step()
    before = planes(sim)
    assert all(before.planes[c][before.planes[c] != (er.NEVER if c == er.ARRIVAL else 0)].size for c in er.CHANNELS)
    # a get / set round trip on every channel, through another handle's planes
    other = load("flume").set_envelope(ea.ENV_ALL)
    for c in er.CHANNELS:
        other.set_envelope_field(c, before.planes[c])
    assert_planes(planes(other), before, "the round trip")
    assert other.envelope() == (ea.ENV_ALL, 0)
    other.close()
    # a disabled channel is freed, the rest keep their words
    assert grows(ea.ENV_ARRIVAL | ea.ENV_PRESSURE) == -2 * plane
    assert_bits(sim.envelope_field(ea.ENV_PRESSURE).view(np.uint32), before.planes[er.PRESSURE], "pressure behind disabling others")
    assert_bits(sim.envelope_field(ea.ENV_ARRIVAL).view(np.uint32), before.planes[er.ARRIVAL], "arrival behind disabling others")
    sim.envelope_reset()
    assert sim.envelope() == (ea.ENV_ARRIVAL | ea.ENV_PRESSURE, 0)
    assert (sim.envelope_field(ea.ENV_ARRIVAL).view(np.uint32) == er.NEVER).all() and not sim.envelope_field(ea.ENV_PRESSURE).view(np.uint32).any()
    assert grows(0) == -(plane + p_plane) and sim.envelope() == (0, 0)
    # every load switches it off and frees the planes: switching it on again allocates all four
    snap, sess = str(tmp_path / "s.snap"), str(tmp_path / "s.sess")
    sim.save_state(snap); sim.save_session(sess)
    size, text, up = scene("flume")
    for again in (lambda: sim.load_text(text, upscale=up), lambda: sim.load_half_tank(), lambda: sim.load_state(snap), lambda: sim.load_session(sess)):
        assert grows(ea.ENV_ALL) == 3 * plane + p_plane
        sim.step()
        assert sim.envelope()[0] == ea.ENV_ALL and sim.envelope()[1] > 0
        b0 = sim.hbm_bytes()
        again()
        assert sim.envelope() == (0, 0) and b0 - sim.hbm_bytes() == 3 * plane + p_plane
        sim.step()
    sim.close()
    probe = load("flume")      # euler_destroy releases the planes with everything else: nothing to assert here but that it returns
    probe.set_envelope(ea.ENV_ALL)
    probe.close()


def _rc(fn, *args):
    return fn(*args), ea.load_library().euler_last_error().decode()


def test_refusals_in_their_order():
    L = ea.load_library()
    Xg, Yg = 100, 40
    n = Xg * Yg
    buf = np.zeros(n, np.float32)
    px = np.zeros(4, ea.ENVELOPE_PX_DTYPE)
    ch, sub = C.c_uint32(7), C.c_uint64(7)
    calls = {      # name -> the call on a handle pointer h with otherwise good arguments
        "set": lambda h: L.euler_set_envelope(h, ea.ENV_WET),
        "get": lambda h: L.euler_get_envelope(h, C.byref(ch), C.byref(sub)),
        "reset": lambda h: L.euler_envelope_reset(h),
        "get_field": lambda h: L.euler_envelope_get_field(h, ea.ENV_WET, buf.ctypes.data, buf.nbytes),
        "set_field": lambda h: L.euler_envelope_set_field(h, ea.ENV_WET, buf.ctypes.data, buf.nbytes),
        "raster": lambda h: L.euler_envelope_raster(h, 1, 1, 4, 4, 2, 2, px.ctypes.data, px.nbytes),
    }
    # 1. a null handle or pointer
    for name, call in calls.items():
        assert call(None) == EULER_EINVAL, name
    sim = ea.Simulation(Xg, Yg)
    assert L.euler_envelope_get_field(sim.h, ea.ENV_WET, None, buf.nbytes) == EULER_EINVAL
    assert L.euler_envelope_set_field(sim.h, ea.ENV_WET, None, buf.nbytes) == EULER_EINVAL
    assert L.euler_envelope_raster(sim.h, 1, 1, 4, 4, 2, 2, None, px.nbytes) == EULER_EINVAL
    # 2. a row-slab handle, before "nothing loaded" and before the arguments
    slab = ea.Simulation(Xg, 128, slab=(0, 1))
    base_slab = slab.hbm_bytes()
    for name, call in calls.items():
        rc, msg = _rc(call, slab.h)
        assert rc == EULER_ESTATE and "slab" in msg, (name, rc, msg)
    assert L.euler_set_envelope(slab.h, 99) == EULER_ESTATE and slab.hbm_bytes() == base_slab
    slab.close()
    # 3. nothing loaded
    base = sim.hbm_bytes()
    for name, call in calls.items():
        rc, msg = _rc(call, sim.h)
        assert rc == EULER_ESTATE and "loaded" in msg, (name, rc, msg)
    assert L.euler_set_envelope(sim.h, 99) == EULER_ESTATE and sim.hbm_bytes() == base
    # 4. the arguments
    size, text, up = scene("waterfall")
    sim.load_text(text, upscale=up)
    base = sim.hbm_bytes()
    for bad in (16, 31, 1 << 31):
        assert L.euler_set_envelope(sim.h, bad) == EULER_EINVAL
    assert sim.envelope() == (0, 0) and sim.hbm_bytes() == base
    assert calls["get_field"](sim.h) == EULER_EINVAL      # the envelope is off: no channel is enabled
    sim.set_envelope(ea.ENV_ARRIVAL | ea.ENV_WET | ea.ENV_PRESSURE)
    sim.step()
    before = planes(sim)
    for fn in (L.euler_envelope_get_field, L.euler_envelope_set_field):
        for bad in (0, ea.ENV_SPEED, ea.ENV_ARRIVAL | ea.ENV_WET, ea.ENV_ALL, 16, -1):      # not exactly one enabled bit
            assert fn(sim.h, bad, buf.ctypes.data, buf.nbytes) == EULER_EINVAL, bad
        for bad in (0, buf.nbytes - 4, buf.nbytes + 4):
            assert fn(sim.h, ea.ENV_WET, buf.ctypes.data, bad) == EULER_EINVAL, bad
    # set_field's bad words: the first bad index is named and the plane stays
    good = {c: before.planes[c].copy().reshape(-1) for c in before.planes}
    words = {"-0.f": 0x80000000, "a negative": np.array(-1.0, np.float32).view(np.uint32), "inf": 0x7F800000, "a NaN": 0x7FC00000, "never": 0xFFFFFFFF}
    for c in before.planes:
        for what, w in words.items():
            if c == er.ARRIVAL and what == "never":
                continue
            src = good[c].copy()
            src[1234], src[3000] = w, w
            rc, msg = _rc(L.euler_envelope_set_field, sim.h, c, src.ctypes.data, src.nbytes)
            assert rc == EULER_EINVAL and "word 1234 " in msg, (c, what, rc, msg)
    assert_planes(planes(sim), before, "behind the refused calls")
    # the raster: the box, W, H and the size, as euler_overview_box
    rast = lambda x0, y0, x1, y1, W, H, nbytes: L.euler_envelope_raster(sim.h, x0, y0, x1, y1, W, H, px.ctypes.data, nbytes)
    for box in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, Xg - 1, 4), (1, 1, 4, Yg - 1), (5, 1, 4, 4), (1, 5, 4, 4)):
        assert rast(*box, 1, 1, 32) == EULER_EINVAL, box
    for W, H, nbytes in ((0, 1, 0), (1, 0, 0), (5, 1, 160), (1, 5, 160), (2, 2, 96), (2, 2, 160)):
        assert rast(1, 1, 4, 4, W, H, nbytes) == EULER_EINVAL, (W, H, nbytes)
    assert rast(1, 1, 4, 4, 2, 2, 128) == 0
    assert sim.hbm_bytes() >= base
    sim.close()


# ----------------------------------------------------------------------------- the raster
@pytest.mark.parametrize("name", ["waterfall", "flume", "wide"])
def test_raster_against_numpy(name):
    sim = load(name)
    rng = np.random.default_rng(len(name))
    Xg, Yg = sim.X, sim.Y
    for channels in (ea.ENV_ALL, ea.ENV_WET | ea.ENV_PRESSURE, ea.ENV_ARRIVAL, 0):
        sim.set_envelope(0).set_envelope(channels)
        for _ in range(6):
            sim.step()
        env = planes(sim) if channels else er.Envelope(Xg, Yg, 0)
        whole = (1, 1, Xg - 2, Yg - 2)
        cases = [(whole, 1, 1), (whole, 7, 3)]      # one pixel for the whole interior
        if channels == ea.ENV_ALL:
            cases.append((whole, Xg - 2, Yg - 2))      # one pixel per cell
        for _ in range(8):
            x0, y0 = int(rng.integers(1, Xg - 2)), int(rng.integers(1, Yg - 2))
            x1, y1 = int(rng.integers(x0, Xg - 1)), int(rng.integers(y0, Yg - 1))
            cases.append(((x0, y0, x1, y1), int(rng.integers(1, x1 - x0 + 2)), int(rng.integers(1, y1 - y0 + 2))))
        for box, W, H in cases:
            got, want = sim.envelope_raster(box, W, H), er.raster(env, box, W, H)
            assert got.tobytes() == want.tobytes(), (name, channels, box, W, H)
        if channels == ea.ENV_ALL:
            one = sim.envelope_raster(whole, 1, 1)[0, 0]
            assert one["touched"] > 0 and one["cells"] == (Xg - 2) * (Yg - 2) and one["arrival_min"] < one["arrival_max"] < 0x7F800000
            assert one["wet_max"] > 0 and one["speed2_max"] > 0 and (one["p_max"] > 0 or name == "waterfall")      # (the waterfall's water is still falling: no pressure yet)
    sim.close()
