"""Passive tracers on the GPU (docs/tracers.md): every word of every record against the restatement (tests/tracers_ref.py; pinned on the CPU by
test_tracers_host.py), bit for bit - one stage from an uploaded oracle state for every launch shape, free runs with the tracers of a streakline added while
they run, a tracer that shadows marker 0; that the tracers leave no trace in the state and add exactly one launch per substep; retirement in a wall and in
a sink; the store, its growth and its refusals; and the raster against numpy, exactly."""
import ctypes as C

import numpy as np
import pytest

import edit_ref
import euler_amd as ea
import tracers_ref as tref
from euler_amd import scenarios
from golden_util import X, Y, load, scenario_text
from observer_util import EULER_EINVAL, EULER_ESTATE, STATE_FIELDS, no_trace_pair
from oracle_lib import Oracle
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(100, 40),      # the reference's scenarios
         (103, 41),      # ragged
         (264, 136)]     # 5 x 3 tiles
COUNTS = (1, 63, 64, 65, 255, 256, 257, 4099)      # a lane, a wave and a workgroup, each one short, full and one over; seventeen workgroups
FREE_FRAMES, WALL_FRAME, TRACKED_FRAMES = 20, 8, 12
WORDS = ea.TRACER_DTYPE.names


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return tref.build(tmp_path_factory.mktemp("tracers"))


def assert_records(got, want, what):
    assert got.shape == want.shape, what
    for w in WORDS:
        a, b = np.ascontiguousarray(got[w]).view(np.uint32), np.ascontiguousarray(want[w]).view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert not len(bad), "%s: word %s of record %d: %r, the restatement %r (%d records differ)" % (what, w, bad[0], got[w][bad[0]], want[w][bad[0]], len(bad))


# ----------------------------------------------------------------------------- scenes (test_tracers_host.py checks on the oracle what the tests below rely on)
def flume_text():
    """a 95 x 38 picture: a walled box, a column of water standing on the floor at the left that collapses at once, four sink cells on the floor a few columns in front
    of it and a low wall further on"""
    w, h = 95, 38
    g = [[" "] * w for _ in range(h)]
    for x in range(w):
        g[0][x] = g[h - 1][x] = "X"
    for y in range(h):
        g[y][0] = g[y][w - 1] = "X"
    for y in range(12, 37):
        for x in range(2, 41):
            g[y][x] = "0"
    for y in range(31, 37):
        g[y][60] = g[y][61] = "X"
    for y in range(35, 37):
        for x in range(46, 50):
            g[y][x] = "="
    return "\n".join("".join(r) for r in g) + "\n"


def free_run_oracle(Xg, Yg):
    return Oracle(Xg, Yg).load_text(flume_text(), upscale=True)


def wall_box(rec, Xg, Yg):
    """3 x 3 cells around a live tracer in the water (the one in the middle of them by x): where a wall is raised over live tracers"""
    live = np.flatnonzero((rec["flags"] & (ea.TRACER_RETIRED | ea.TRACER_WET)) == ea.TRACER_WET)
    k = live[np.argsort(rec["x"][live], kind="stable")[len(live) // 2]]
    cx, cy = int(np.floor(rec["x"][k])), int(np.floor(rec["y"][k]))
    x0, y0 = min(max(cx - 1, 1), Xg - 4), min(max(cy - 1, 1), Yg - 4)
    return (x0, y0, x0 + 2, y0 + 2)


def raise_wall(o, box):
    """euler_edit_box(EULER_EDIT_SOLID) on the oracle (tests/edit_ref.py)"""
    x0, y0, x1, y1 = box
    sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    o.solid[sl] = 1
    o.sink[sl] = 0
    o.source[sl] = 0
    o.set_markers(edit_ref.delete_in_box_vectorised(o.markers, box))
    o.count[sl] = 0


def special_points(o):
    """points in air, in a solid cell, in an interior sink cell, on cell edges and one ulp either side of them, at 1.0 and just below X - 1 / Y - 1"""
    Xg, Yg = o.X, o.Y
    up, down = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))
    inner = np.zeros((Yg, Xg), bool)
    inner[1:-1, 1:-1] = True
    wet = np.argwhere((o.count > 0) & inner)
    air = np.argwhere((o.count == 0) & (o.solid == 0) & (o.sink == 0) & inner)
    sol = np.argwhere((o.solid != 0) & inner)
    snk = np.argwhere((o.sink != 0) & inner)
    pts = [(x + 0.5, y + 0.5) for y, x in air[:: max(1, len(air) // 6)][:6]]
    pts += [(x + 0.25, y + 0.5) for y, x in sol[:: max(1, len(sol) // 4)][:4]]
    pts += [(x + 0.75, y + 0.25) for y, x in snk[:2]]
    for y, x in wet[:: max(1, len(wet) // 5)][:5]:
        pts += [(F32(x), y + 0.5), (up(x), y + 0.5), (down(x + 1), y + 0.5), (x + 0.5, F32(y)), (x + 0.5, up(y)), (x + 0.5, down(y + 1)), (F32(x), F32(y))]
    pts += [(1.0, 1.0), (down(Xg - 1), 1.0), (1.0, down(Yg - 1)), (down(Xg - 1), down(Yg - 1)), (down(Xg - 1), Yg // 2 + 0.5)]
    return np.array(pts, F32)


def water_lattice(o, k=2, limit=None):
    """the k x k lattice of every wet interior cell, x outer"""
    wet = (o.count > 0)
    wet[0, :] = wet[-1, :] = wet[:, 0] = wet[:, -1] = False
    cells = np.argwhere(wet.T)      # x outer, y inner
    if limit and len(cells) * k * k > limit:
        cells = cells[:: -(-len(cells) * k * k // limit)]
    return np.concatenate([ea.tracer_lattice((x, y, x, y), k) for x, y in cells])


def free_run_tracers(o):
    return np.concatenate([special_points(o), water_lattice(o, 2, 360)])


def emit_points(Xg, Yg):
    """three points of a streakline: a tracer is added at each before every frame"""
    return np.array([[Xg * 0.38, Yg * 0.2], [Xg * 0.2, Yg * 0.5], [Xg * 0.7, Yg * 0.8]], F32)


def tracked_scene_oracle():
    """a closed box (no source, no sink inside): the marker count stays, markers[0] is never moved by a deletion"""
    return Oracle(X, Y).load_text(scenarios.dam_break(), upscale=True)


def upload(sim, o):
    """the oracle's state into a handle that loaded the same scene"""
    for f, a in ((ea.F_SOLID, o.solid), (ea.F_SOURCE, o.source), (ea.F_SINK, o.sink), (ea.F_U, o.u), (ea.F_V, o.v), (ea.F_UTMP, o.utmp), (ea.F_VTMP, o.vtmp),
                 (ea.F_COUNT, o.count), (ea.F_PREV_COUNT, o.prev_count), (ea.F_PRECON, o.precon)):
        sim.set(f, a)
    sim.set_markers(o.markers)
    sim.set_rng(int(o.c.rng_state), int(o.c.source_exhausted))


# ----------------------------------------------------------------------------- one stage, teacher-forced
def _stage_scene(which):
    if which == "waterfall":
        text = scenario_text(load("waterfall_frames.npz"))
        return (X, Y), text, False
    return (103, 41), flume_text(), True


@pytest.mark.parametrize("which", ["waterfall", "flume"])
@pytest.mark.parametrize("frame", [0, 6])
def test_teacher_forced_stage(libs, which, frame):
    """euler_stage(ADVECT_MARKERS) from the oracle's state at frames 0 and 6: all eight words of every record equal the restatement, for every launch shape
    of COUNTS, three values of dt, RK1 and RK2; the markers move as they do without tracers"""
    am, tw = libs
    size, text, upscale = _stage_scene(which)
    o = Oracle(*size).load_text(text, upscale=upscale)
    for _ in range(frame):
        o.step()
    base = np.concatenate([special_points(o), water_lattice(o, 2)])
    xy = np.resize(base, (max(COUNTS), 2))      # (cyclic: the list again where it is shorter)
    cfl = o.timestep(0.1)
    sim = ea.Simulation(*size, dot_mode=ea.DOT_SEQUENTIAL).load_text(text, upscale=upscale)
    upload(sim, o)
    m0 = o.markers.copy()
    seen = 0
    for rk2 in (False, True):
        sim.set_option(ea.OPT_ADVECT_RK2, int(rk2))
        for dt in (cfl, float(F32(cfl) * F32(0.37)), 0.001):
            want = tref.tracer_substep(tw, o, tref.records(xy), dt, rk2)
            o.set_markers(m0)
            tref.rk2ref.advect_markers(am, o, dt, rk2)
            m1 = o.markers.copy()
            o.set_markers(m0)
            for n in COUNTS:
                sim.clear_tracers().add_tracers(xy[:n])
                sim.set_markers(m0)
                sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
                assert sim.n_tracers == n
                assert_records(sim.tracers(), want[:n], "%s frame %d rk2 %d dt %g n %d" % (which, frame, rk2, dt, n))
                assert_bits(sim.get(ea.F_MARKERS), m1, "markers next to %d tracers" % n)
            fl = want["flags"]
            seen |= int(np.bitwise_or.reduce(fl))
            assert (want["substeps"] == ((fl & ea.TRACER_RETIRED) == 0)).all()
    assert seen == ea.TRACER_WET | ea.TRACER_RETIRED | ea.TRACER_IN_SOLID | ea.TRACER_IN_SINK | ea.TRACER_WAS_DRY      # (LOST needs a position add refuses)
    sim.close()


# ----------------------------------------------------------------------------- free runs
def free_run_script(libs, size, mode):
    """The free run on the oracle, as the events a handle replays: ("add", positions), ("wall", box) - euler_edit_box(SOLID) over live tracers at WALL_FRAME -
    and ("frame", f, records after it, clock, oracle).  Three tracers of a streakline are added before every frame."""
    rk2, mc = mode != "rk1", mode.startswith("maccormack")
    o = free_run_oracle(*size)
    xy = free_run_tracers(o)
    rec = tref.records(xy)
    yield ("add", xy)
    clock = 0.0
    for f in range(FREE_FRAMES):
        e = emit_points(*size)
        rec = np.concatenate([rec, tref.records(e)])
        yield ("add", e)
        if f == WALL_FRAME:
            box = wall_box(rec, *size)
            raise_wall(o, box)
            yield ("wall", box)
        clock = tref.step(libs, o, rec, rk2=rk2, mc=mc, clock=clock)
        yield ("frame", f, rec.copy(), clock, o)


def in_box(rec, box):
    return (np.floor(rec["x"]) >= box[0]) & (np.floor(rec["x"]) <= box[2]) & (np.floor(rec["y"]) >= box[1]) & (np.floor(rec["y"]) <= box[3])


@pytest.mark.parametrize("mode", ["rk1", "rk2", "maccormack+rk2"])
@pytest.mark.parametrize("size", SIZES)
def test_free_run(libs, size, mode):
    """20 frames: the records after every frame, with three tracers of a streakline added before each and a wall raised over live tracers at WALL_FRAME;
    the state and the clock are the composition's"""
    sim = ea.Simulation(*size, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
    sim.set_option(ea.OPT_ADVECT_RK2, int(mode != "rk1")).set_option(ea.OPT_ADVECT_MACCORMACK, int(mode.startswith("maccormack")))
    before = inbox = None
    for ev in free_run_script(libs, size, mode):
        if ev[0] == "add":
            sim.add_tracers(ev[1])
        elif ev[0] == "wall":
            before = sim.tracers()
            inbox = ((before["flags"] & ea.TRACER_RETIRED) == 0) & in_box(before, ev[1])
            assert inbox.sum() >= 1
            sim.edit_box(ea.EDIT_SOLID, ev[1])
        else:
            _, f, rec, clock, o = ev
            sim.step()
            assert_records(sim.tracers(), rec, "%r %s frame %d" % (size, mode, f))
            assert sim.time == clock
            if f == WALL_FRAME:      # the live tracers of the box retired on the next substep, where they were, with IN_SOLID
                assert ((rec["flags"][inbox] & ea.TRACER_IN_SOLID) != 0).all()
                assert np.array_equal(rec["x"][inbox], before["x"][inbox]) and (rec["substeps"][inbox] == before["substeps"][inbox]).all()
    for fld, want in ((ea.F_U, o.u), (ea.F_V, o.v), (ea.F_COUNT, o.count), (ea.F_MARKERS, o.markers)):
        assert_bits(sim.get(fld), want, "%r %s field %d" % (size, mode, fld))
    assert int(sim.stats().rng_state) == int(o.c.rng_state)
    fl = rec["flags"]
    assert ((fl & ea.TRACER_IN_SINK) != 0).any() and ((fl & ea.TRACER_IN_SOLID) != 0).any()
    sim.close()


def test_a_tracer_at_marker_0_is_marker_0():
    """marker 0 always gets the full dt and, in a scene whose marker count stays, keeps its place in the array: a tracer added on it shadows it bit for bit"""
    for rk2 in (0, 1):
        sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenarios.dam_break(), upscale=True)
        sim.set_option(ea.OPT_ADVECT_RK2, rk2)
        n0 = sim.stats().n_markers
        sim.add_tracers(sim.get(ea.F_MARKERS)[:1])
        moved = False
        for f in range(TRACKED_FRAMES):
            before = sim.get(ea.F_MARKERS)[0].copy()
            sim.step()
            t, m = sim.tracers()[0], sim.get(ea.F_MARKERS)[0]
            assert sim.stats().n_markers == n0
            assert_bits(np.array([t["x"], t["y"]], F32), m, "rk2 %d frame %d" % (rk2, f))
            moved |= not np.array_equal(before, m)
        assert moved and sim.tracers()[0]["path"] > 0
        sim.close()


# ----------------------------------------------------------------------------- no trace, launch accounting
def _no_trace(size, options=(), frames=20, **kw):
    def make():
        s = ea.Simulation(*size, **kw).load_text(flume_text(), upscale=True)
        for k, v in options:
            s.set_option(k, v)
        return s

    state = {"calls": 0}

    def look(s, stepped):
        state["calls"] += 1
        if state["calls"] % 3 == 1:
            s.add_tracers(ea.tracer_lattice((size[0] * 10 // 100, 3, size[0] * 10 // 100 + 4, 6), 2))
        s.add_tracers(emit_points(*size)[:1])
        n = s.n_tracers
        assert len(s.tracers()) == n and len(s.tracers(n // 2, n - n // 2)) == n - n // 2
        assert s.tracer_raster(None, 9, 7, all=True).sum() == n
        s.tracer_raster((2, 2, size[0] // 2, size[1] // 2), 3, 2)

    a, b = no_trace_pair(make, look, None, STATE_FIELDS, frames)
    rec = b.tracers()
    assert a.n_tracers == 0 and len(rec) > 100 and (rec["substeps"] > 0).sum() > 100 and (rec["path"] > 0).any()
    a.close(); b.close()


def test_tracers_leave_no_trace():
    _no_trace((100, 40), dot_mode=ea.DOT_SEQUENTIAL)


@pytest.mark.parametrize("resident", [ea.RESIDENT_AUTO, ea.RESIDENT_OFF])
def test_no_trace_with_the_tile_solver(resident):
    _no_trace((264, 136), dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, resident=resident, max_iterations=50)


def test_no_trace_without_the_lean_passes():
    _no_trace((103, 41), options=((ea.OPT_NO_TILE_MAP, 1), (ea.OPT_MARKERS_TWO_PASS, 1), (ea.OPT_BUILD_TWO_PASS, 1), (ea.OPT_VELOCITY_TWO_PASS, 1)), dot_mode=ea.DOT_SEQUENTIAL)


def test_launch_accounting():
    """every profile class over 3 frames: add then clear launches what a handle that called nothing launches; with tracers, one more marker_advect launch per substep"""
    names = ea.profile_class_names()

    def run(prepare):
        s = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
        prepare(s)
        s.profile_enable(names)
        s.profile_reset()
        for _ in range(3):
            s.step()
        prof = {k: v[1] for k, v in s.profile().items()}
        sub = int(s.stats().total_substeps)
        s.close()
        return prof, sub

    plain, sub = run(lambda s: None)
    cleared, sub2 = run(lambda s: s.add_tracers(ea.tracer_lattice((5, 5, 8, 8), 2)).clear_tracers())
    traced, sub3 = run(lambda s: s.add_tracers(ea.tracer_lattice((5, 5, 8, 8), 2)))
    assert sub == sub2 == sub3 >= 3
    assert cleared == plain
    want = dict(plain)
    want["marker_advect"] += sub
    assert traced == want


# ----------------------------------------------------------------------------- retirement
def test_a_retired_record_never_changes_again(libs):
    """tracers in a wall, in the sink and carried into the sink: retired where they were, and the same bytes twenty substeps on"""
    o = free_run_oracle(X, Y)
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
    xy = free_run_tracers(o)
    sim.add_tracers(xy)
    seen = {}
    for f in range(FREE_FRAMES):
        sim.step()
        rec = sim.tracers()
        for k in np.flatnonzero(rec["flags"] & ea.TRACER_RETIRED):
            if k in seen:
                assert rec[k].tobytes() == seen[k], (f, k)
            else:
                seen[k] = rec[k].tobytes()
    rec = sim.tracers()
    carried = ((rec["flags"] & ea.TRACER_IN_SINK) != 0) & (rec["substeps"] > 0)
    assert carried.sum() >= 1 and len(seen) > carried.sum()
    snk = sim.get(ea.F_SINK)
    assert (snk[np.floor(rec["y"][carried]).astype(int), np.floor(rec["x"][carried]).astype(int)] != 0).all()      # its last position: the sink cell it was carried into
    first = ((rec["flags"] & (ea.TRACER_IN_SINK | ea.TRACER_IN_SOLID)) != 0) & (rec["substeps"] == 0)      # added inside a wall or the sink: accepted, retired on the first substep
    assert first.sum() >= 4 and np.array_equal(rec["x"][first], xy[first, 0]) and (rec["age"][first] == 0).all()
    sim.close()


def test_a_wall_raised_over_tracers_retires_exactly_those_in_the_box():
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
    o = free_run_oracle(X, Y)
    sim.add_tracers(water_lattice(o, 2, 1200))
    for _ in range(3):
        sim.step()
    before = sim.tracers()
    box = wall_box(before, X, Y)
    sim.edit_box(ea.EDIT_SOLID, box)
    assert sim.tracers().tobytes() == before.tobytes()      # the edit itself leaves them alone
    sim.substep(sim.timestep(0.1))
    rec = sim.tracers()
    inbox = in_box(before, box)
    assert 3 <= inbox.sum() < len(rec) and not (before["flags"] & ea.TRACER_RETIRED).any()
    assert np.array_equal((rec["flags"] & ea.TRACER_RETIRED) != 0, inbox)
    assert (rec["flags"][inbox] == (before["flags"][inbox] | ea.TRACER_RETIRED | ea.TRACER_IN_SOLID)).all()
    for w in ("x", "y", "path", "age", "wet_time", "substeps"):
        assert np.array_equal(rec[w][inbox], before[w][inbox]), w
    assert (rec["substeps"][~inbox] == before["substeps"][~inbox] + 1).all()
    sim.close()


# ----------------------------------------------------------------------------- the store
def test_store_growth_clear_and_loads():
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
    sim.step()      # (the solver's lazily allocated arrays come with the first solve)
    base = sim.hbm_bytes()
    rng = np.random.default_rng(1)
    assert sim.n_tracers == 0 and len(sim.tracers()) == 0
    sim.add_tracers(np.zeros((0, 2), F32))
    assert sim.n_tracers == 0 and sim.hbm_bytes() == base      # n == 0: a no-op
    all_xy = np.zeros((0, 2), F32)
    sizes = []
    for n in (10, 200, 300, 7, 1500):      # 256 records first, then 512, 1024, 2048: the five calls cross the growths with records in the store
        xy = np.stack([rng.uniform(1, X - 1.001, n), rng.uniform(1, Y - 1.001, n)], 1).astype(F32)
        sim.step()      # (the records so far are no longer fresh)
        before = sim.tracers()
        sim.add_tracers(xy)
        all_xy = np.concatenate([all_xy, xy])
        rec = sim.tracers()
        assert rec[: len(before)].tobytes() == before.tobytes()      # growth keeps the records bit for bit
        assert rec[len(before):].tobytes() == tref.records(xy).tobytes()      # the new ones: their position, all other words 0
        sizes.append(sim.hbm_bytes() - base)
    assert sizes == [256 * 32, 256 * 32, 512 * 32, 1024 * 32, 2048 * 32]      # the buffer and nothing else; it doubles
    assert sim.n_tracers == len(all_xy) == 2017
    sim.tracer_raster(None, 4, 3)
    grown = sim.hbm_bytes()
    assert grown == base + 2048 * 32 + 4 * 3 * 4
    sim.clear_tracers()
    assert sim.n_tracers == 0 and sim.hbm_bytes() == grown and not sim.tracer_raster(None, 4, 3, all=True).any()      # n = 0, the buffer stays
    sim.add_tracers(all_xy[:5])
    assert sim.tracers().tobytes() == tref.records(all_xy[:5]).tobytes() and sim.hbm_bytes() == grown
    # every load clears: the tracers belonged to the run that was replaced
    for load_again in (lambda: sim.load_text(flume_text(), upscale=True), lambda: sim.load_half_tank()):
        sim.add_tracers(all_xy[:5])
        assert sim.n_tracers > 0
        load_again()
        assert sim.n_tracers == 0
    sim.close()


def test_load_state_clears_and_the_setters_do_not(tmp_path):
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
    sim.step()
    snap = str(tmp_path / "state.snap")
    sim.save_state(snap)
    sim.add_tracers([[10.5, 5.5], [20.5, 6.5]])
    sim.step()
    want = sim.tracers().tobytes()
    sim.set(ea.F_U, sim.get(ea.F_U)); sim.set_markers(sim.get(ea.F_MARKERS)); sim.edit_box(ea.EDIT_CLEAR, (60, 20, 61, 21)); sim.set_forcing((0.0, -10.0)); sim.time = 1.5
    assert sim.n_tracers == 2 and sim.tracers().tobytes() == want
    sim.load_state(snap)
    assert sim.n_tracers == 0
    sim.close()


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    L = ea.load_library()
    one = np.array([[5.5, 5.5]], F32)
    assert L.euler_tracers_add(None, one.ctypes.data, 1) == EULER_EINVAL      # 1: a null handle
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:      # 2: a row-slab handle, before "nothing loaded"
        slab.add_tracers(one)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL)
    base = sim.hbm_bytes()
    with pytest.raises(ea.EulerError) as e:      # 3: nothing loaded, before the list is looked at
        sim.add_tracers([[np.nan, 0.0]])
    assert e.value.code == EULER_ESTATE and "loaded" in str(e.value)
    with pytest.raises(ea.EulerError) as e:
        sim.tracer_raster(None, 4, 4)
    assert e.value.code == EULER_ESTATE
    sim.load_text(flume_text(), upscale=True)
    sim.add_tracers([[5.5, 5.5], [6.5, 5.5], [7.5, 5.5]])
    base = sim.hbm_bytes()
    want = sim.tracers().tobytes()

    def refused(call, code, word):
        with pytest.raises(ea.EulerError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert sim.n_tracers == 3 and sim.hbm_bytes() == base and sim.tracers().tobytes() == want      # a refused call changes and allocates nothing

    h = sim.h
    refused(lambda: ea._check(L.euler_tracers_add(h, None, 2)), EULER_EINVAL, "null")      # 4
    many = np.full((ea.TRACERS_MAX - 2, 2), 5.5, F32)
    many[7] = np.nan
    refused(lambda: sim.add_tracers(many), EULER_EINVAL, "at most")      # 5: the count, before the positions
    bad = np.array([[5.5, 5.5], [6.5, 5.5], [0.5, 5.5], [np.nan, 5.5]], F32)
    refused(lambda: sim.add_tracers(bad), EULER_EINVAL, "tracer 2:")      # 6: the first such index
    for p in ((np.nan, 5.0), (5.0, np.inf), (0.999, 5.0), (5.0, 0.0), (X - 1.0, 5.0), (5.0, Y - 1.0), (-7.0, 5.0), (1e30, 5.0)):
        refused(lambda: sim.add_tracers([p]), EULER_EINVAL, "tracer 0:")
    sim.add_tracers([[1.0, 1.0], [np.nextafter(F32(X - 1), F32(0)), np.nextafter(F32(Y - 1), F32(0))]])      # the bounds themselves
    assert sim.n_tracers == 5
    sim.clear_tracers().add_tracers([[5.5, 5.5], [6.5, 5.5], [7.5, 5.5]])
    # get: bad ranges and byte counts; n == 0 succeeds
    out = np.zeros(4, ea.TRACER_DTYPE)
    for first, n, nbytes in ((0, 4, 128), (3, 1, 32), (4, 0, 0), (1, 2, 32), (0, 3, 97), (2**63, 2**63, 0), (0, 2**64 - 1, 32)):
        assert L.euler_tracers_get(h, first, n, out.ctypes.data, nbytes) == EULER_EINVAL, (first, n, nbytes)
    assert L.euler_tracers_get(h, 3, 0, None, 0) == 0 and L.euler_tracers_get(h, 0, 0, None, 0) == 0 and L.euler_tracers_get(None, 0, 0, None, 0) == EULER_EINVAL
    assert L.euler_tracers_get(h, 1, 2, out.ctypes.data, 64) == 0 and out[:2].tobytes() == sim.tracers()[1:3].tobytes() and len(sim.tracers(1)) == 2
    n = C.c_size_t(9)
    assert L.euler_tracers_count(None, C.byref(n)) == EULER_EINVAL and L.euler_tracers_count(h, None) == EULER_EINVAL and L.euler_tracers_clear(None) == EULER_EINVAL
    # the raster's own checks, behind the observers' entry checks
    ras = np.zeros(16, np.uint32)
    for args in ((0, 1, 5, 5, 1, 1, 0, 4), (1, 1, X - 1, 5, 1, 1, 0, 4), (5, 5, 4, 5, 1, 1, 0, 4), (1, 1, 4, 4, 5, 1, 0, 20), (1, 1, 4, 4, 1, 0, 0, 0), (1, 1, 4, 4, 2, 2, 0, 12),
                 (1, 1, 4, 4, 2, 2, 2, 16), (1, 1, 4, 4, 2, 2, 3, 16), (1, 1, 4, 4, 2, 2, -1, 16)):
        assert L.euler_tracer_raster(h, *args[:7], ras.ctypes.data, args[7]) == EULER_EINVAL, args
    assert L.euler_tracer_raster(h, 1, 1, 4, 4, 2, 2, 0, None, 16) == EULER_EINVAL and L.euler_tracer_raster(None, 1, 1, 4, 4, 2, 2, 0, ras.ctypes.data, 16) == EULER_EINVAL
    assert sim.n_tracers == 3 and sim.tracers().tobytes() == want
    sim.close()


# ----------------------------------------------------------------------------- the raster
def _raster_cases(sim, rec, boxes):
    n = 0
    for box in boxes:
        x0, y0, x1, y1 = box
        Bw, Bh = x1 - x0 + 1, y1 - y0 + 1
        rasters = {(Bw, Bh), (1, 1), (Bw, 1), (1, Bh), (max(Bw // 2, 1), max(Bh // 3, 1)), (max(Bw - 1, 1), max(Bh - 1, 1))}
        for W, H in sorted(rasters):
            for every in (False, True):
                got = sim.tracer_raster(box, W, H, all=every)
                assert got.dtype == np.uint32 and np.array_equal(got, tref.raster(rec, box, W, H, every)), (box, W, H, every)
                n += 1
    return n


@pytest.mark.parametrize("size", SIZES)
def test_raster_against_numpy(size):
    """exactly: the whole interior and boxes with every residue of Bw % W, W = Bw and W = 1, with and without the retired tracers, n = 0, tracers exactly on
    a box's edges; on 264 x 136 with 4099 tracers, many of them in a few cells: several workgroups add into one pixel"""
    Xg, Yg = size
    o = free_run_oracle(Xg, Yg)
    sim = ea.Simulation(Xg, Yg, dot_mode=ea.DOT_SEQUENTIAL).load_text(flume_text(), upscale=True)
    whole = (1, 1, Xg - 2, Yg - 2)
    assert not sim.tracer_raster(whole, Xg - 2, Yg - 2).any() and not sim.tracer_raster((3, 3, 9, 9), 2, 2, all=True).any()      # n = 0: zeros
    rng = np.random.default_rng(size[0])
    xy = np.concatenate([free_run_tracers(o), np.stack([rng.uniform(1, Xg - 1.001, 900), rng.uniform(1, Yg - 1.001, 900)], 1).astype(F32)])
    box = (Xg // 3, 3, Xg // 3 + 12, 3 + 8)      # 13 x 9 cells
    down = lambda v: np.nextafter(F32(v), F32(-np.inf))
    edge = np.array([[box[0], box[1]], [down(box[0]), box[1] + 0.5], [box[2] + 1, box[3] + 0.5], [down(box[2] + 1), down(box[3] + 1)], [box[0] + 0.5, box[3] + 1]], F32)
    xy = np.concatenate([xy, edge])
    if size == (264, 136):
        xy = np.resize(np.concatenate([xy, np.tile(np.array([[40.5, 20.5], [41.25, 20.75], [200.5, 100.5]], F32), (800, 1))]), (4099, 2))
    sim.add_tracers(xy)
    for _ in range(6):      # some retire, the others spread
        sim.step()
    rec = sim.tracers()
    assert ((rec["flags"] & ea.TRACER_RETIRED) != 0).sum() >= 5 and len(rec) == len(xy)
    boxes = [whole, box, (box[0], box[1], box[0], box[1]), (2, 2, Xg - 3, Yg - 3)]
    n = _raster_cases(sim, rec, boxes)
    # every residue of Bw % W on a box of 13 columns, and of Bh % H on its 9 rows
    for W in range(1, 14):
        for H in (1, 4, 9):
            assert np.array_equal(sim.tracer_raster(box, W, H), tref.raster(rec, box, W, H)), (W, H)
    for H in range(1, 10):
        assert np.array_equal(sim.tracer_raster(box, 5, H, all=True), tref.raster(rec, box, 5, H, True)), H
    assert n >= 30
    if size == (264, 136):
        assert len(rec) == 4099 and sim.tracer_raster(whole, 4, 4, all=True).max() > 256      # more than a workgroup's tracers in one pixel
    sim.close()
