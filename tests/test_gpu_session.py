"""Session files on the GPU (docs/session.md): euler_save_session / euler_load_session carry everything a whole-grid handle holds, so that a continued run equals the
uninterrupted one bit for bit - the waterfall with a forcing, heat, tracers, two bodies and the density control at once, under every transport, with the dye, with
viscosity, in the tile-local and the multilevel mode; between two substeps; a plain file switches the extras off; the restore has no switch-on side effects; refused
loads leave the handle alone; euler_load_state takes the core of a session (also into row slabs); versions 1 and 2 are unchanged; and the command line.
Grids 100 x 40, 103 x 41 (ragged) and 264 x 136 (several 64 x 64 tiles).  Every comparison is for equal bits."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import ranks
import session_util as su
from euler_amd import scenarios
from observer_util import EXE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GRIDS = ((100, 40), (103, 41), (264, 136))
FIELDS = (("u", ea.F_U), ("v", ea.F_V), ("utmp", ea.F_UTMP), ("vtmp", ea.F_VTMP), ("solid", ea.F_SOLID), ("source", ea.F_SOURCE), ("sink", ea.F_SINK), ("count", ea.F_COUNT),
          ("prev_count", ea.F_PREV_COUNT), ("precon", ea.F_PRECON), ("markers", ea.F_MARKERS))
DYE = (("dye_r", ea.F_DYE_R), ("dye_g", ea.F_DYE_G), ("dye_b", ea.F_DYE_B), ("dye_rtmp", ea.F_DYE_RTMP), ("dye_gtmp", ea.F_DYE_GTMP), ("dye_btmp", ea.F_DYE_BTMP))
# name -> (constructor arguments, options)
VARIANTS = {
    "plain": ({}, {}),
    "rk2": ({}, {ea.OPT_ADVECT_RK2: 1}),
    "maccormack": ({}, {ea.OPT_ADVECT_MACCORMACK: 1}),
    "maccormack_rk2": ({}, {ea.OPT_ADVECT_MACCORMACK: 1, ea.OPT_ADVECT_RK2: 1}),
    "rainbow": ({"rainbow": True}, {}),
    "viscosity": ({"viscosity": 0.05}, {}),
    "tile_local": ({"precond": ea.PRECOND_IC0_TILE, "tile_records": 16}, {}),
    "multilevel": ({"precond": ea.PRECOND_IC0_TILE_MG, "dot_mode": ea.DOT_TREE, "max_iterations": 400}, {}),
}


def make(X, Y, variant="plain", **more):
    kw, opts = VARIANTS[variant]
    sim = ea.Simulation(X, Y, **dict({"dot_mode": ea.DOT_SEQUENTIAL}, **dict(kw, **more)))
    for k, v in opts.items():
        sim.set_option(k, v)
    return sim


def waterfall(sim):
    return sim.load_text(scenarios.waterfall(), upscale=True)


def everything(sim):
    """the waterfall with every extra on: a tilted, shaken tank with two pumps across the 63 | 64 tile edge, heat with a FIX and a RATE box, two bodies (one oscillating
    under the source, one clamped at the right border), 40 tracers of which four stand in a wall and four in the sink, and the density control"""
    X, Y = sim.X, sim.Y
    waterfall(sim)
    sim.set_forcing(gravity=(1.5, -9.5), shake=(2.0, 0.5, 0.5, 0.3),
                    boxes=[((60, 2, 67, min(6, Y - 2)), (3.0, 0.5)), ((58, max(1, min(60, Y - 9)), 70, min(67, Y - 2)), (-2.0, 1.0))])
    sim.set_heat(ambient=0.0, beta=0.5, kappa=0.3, source_t=8.0, boxes=[(ea.HEAT_FIX, 16.0, (2, Y - 10, 12, Y - 6)), (ea.HEAT_RATE, 5.0, (10, Y - 12, 24, Y - 7))])
    sim.set_bodies([ea.body((3, 2), (8.0, Y - 8.0), amplitude=(3.0, 0.0), hz=0.5), ea.body((2, 2), (X - 5.0, 5.0), velocity=(4.0, 0.0))])
    solid, sink = sim.get(ea.F_SOLID), sim.get(ea.F_SINK)
    inner = np.zeros_like(solid, bool)
    inner[1:-1, 1:-1] = True
    walls, drains = np.argwhere((solid != 0) & inner)[:4], np.argwhere((sink != 0) & inner)[:4]
    assert len(walls) == 4 and len(drains) == 4
    xs, ys = np.meshgrid(np.linspace(2.5, 20.5, 8), np.linspace(Y - 7.5, Y - 2.5, 4))
    xy = np.concatenate([np.stack([xs.ravel(), ys.ravel()], 1), walls[:, ::-1] + 0.5, drains[:, ::-1] + 0.5]).astype(F32)
    assert len(xy) == 40
    sim.add_tracers(xy)
    # forty markers more in one cell of the source's water: the first pass has a crowded cell to thin, so the totals are not zero at any save
    cells = np.argwhere((sim.get(ea.F_SOURCE) != 0) & (sim.get(ea.F_COUNT) != 0) & (solid == 0))
    cy, cx = cells[len(cells) // 2]
    crowd = np.random.default_rng(3).random((40, 2)).astype(F32) * F32(0.875) + np.array([cx, cy], F32)
    sim.set_markers(np.concatenate([sim.get(ea.F_MARKERS).reshape(-1, 2), crowd]))
    sim.set_reseed(thin_above=16, fill_holes=True)
    return sim


def something_else(sim):
    """another scenario with its own, different extras: what a session load has to replace"""
    sim.load_half_tank()
    sim.set_forcing(gravity=(-2.0, -7.0), boxes=[((3, 3, 9, 9), (1.0, 1.0))])
    sim.set_heat(ambient=3.0, beta=0.1, boxes=[(ea.HEAT_FIX, 7.0, (2, 2, 6, 6))])
    sim.add_tracers(np.array([[5.5, 5.5], [6.5, 7.5], [9.25, 3.5]], F32))
    sim.set_bodies([ea.body((2, 3), (20.0, 6.0), velocity=(1.0, 0.0))])
    sim.set_reseed(thin_above=12)
    sim.step()
    return sim


def state(sim, dye=False, heat=True, events=True):
    """everything a session promises, as bytes (events=False: without the two marker event totals, which only a session carries)"""
    s = {n: sim.get(f).tobytes() for n, f in FIELDS + (DYE if dye else ())}
    t = sim.stats()
    s["stats"] = repr([(n, getattr(t, n)) for n, _ in ea.Stats._fields_ if events or n not in ("marker_dt_events", "marker_multi_events")])
    s["time"] = struct.pack("<d", sim.time)
    s["forcing"] = b"".join(a.tobytes() for a in sim.forcing())
    if heat:
        s["heat"] = b"".join(a.tobytes() for a in sim.heat())
        s["T"] = sim.temperature.tobytes()
    s["tracers"] = sim.tracers().tobytes()
    s["bodies"] = b"".join(a.tobytes() for a in sim.bodies())
    s["reseed"] = b"".join(a.tobytes() for a in sim.reseed())
    return s


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def code_of(fn):
    try:
        fn()
    except ea.EulerError as e:
        return e.code, str(e)
    return 0, ""


# ----------------------------------------------------------------------------- 1. everything at once
@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """the plain 100 x 40 run of test 1 up to its save: (file, the state at the save), shared by the tests that only read the file"""
    path = str(tmp_path_factory.mktemp("session") / "all.session")
    a = everything(make(100, 40))
    for _ in range(6):
        a.step()
    a.save_session(path)
    at_save = state(a)
    a.close()
    return path, at_save


@pytest.mark.parametrize("X,Y,variant", [(100, 40, v) for v in VARIANTS] + [(103, 41, "plain"), (264, 136, "plain"), (264, 136, "maccormack_rk2")])
def test_a_continued_run_equals_the_uninterrupted_one(tmp_path, X, Y, variant):
    path = str(tmp_path / "s.session")
    dye = variant == "rainbow"
    a = everything(make(X, Y, variant))
    for _ in range(6):
        a.step()
    a.save_session(path)
    at_save = state(a, dye)
    b = something_else(make(X, Y, variant))
    b.load_session(path)
    assert differing(state(b, dye), at_save) == []      # the handle is in the saving handle's state, whatever it held before
    for _ in range(8):
        a.step(); b.step()
    sa, sb = state(a, dye), state(b, dye)
    assert differing(sa, sb) == []
    # the run was one: the sources fired, tracers retired in the wall and in the sink and others aged with the run, the oscillating body shifted, the pass thinned
    tr, (bodies, now), totals = a.tracers(), a.bodies(), a.reseed()[1]
    assert a.stats().n_markers > 0 and a.stats().frames == 14 and a.time > 1.39
    assert (tr["flags"] & ea.TRACER_IN_SOLID != 0).sum() >= 4 and (tr["flags"] & ea.TRACER_IN_SINK != 0).sum() >= 4 and (tr["age"] > 1.39).any()
    assert len(bodies) == 2 and now["ox"][1] == X - 4 and np.isfinite(a.temperature).all() and np.abs(a.temperature).max() > 0
    assert np.isfinite(a.get(ea.F_U)).all() and np.isfinite(a.get(ea.F_V)).all() and np.abs(a.get(ea.F_V)).max() > 1 and (tr["path"] > 0).any()
    assert sa["markers"] != at_save["markers"] and sa["T"] != at_save["T"]
    assert int(totals["removed"]) >= 24 and int(totals["cells_thinned"]) >= 1      # (the planted cell: 40 markers, at most 16 survive)
    print("reseed totals", {k: int(totals[k]) for k in totals.dtype.names}, "markers", a.stats().n_markers, "retired", int((tr["flags"] & ea.TRACER_RETIRED != 0).sum()), "longest path", float(tr["path"].max()))
    a.close(); b.close()


# ----------------------------------------------------------------------------- 2. between two substeps
def test_a_save_between_two_substeps_continues_by_substeps():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mid.session")
        a = everything(make(103, 41, "rk2"))
        for _ in range(3):
            a.step()
        dts = [F32(0.013), F32(0.021), F32(0.017), F32(0.009), F32(0.025), F32(0.011), F32(0.019)]
        for dt in dts[:3]:
            a.substep(float(dt))
        assert abs(a.time / 0.1 - round(a.time / 0.1)) > 0.05      # off the frame grid
        a.save_session(path)
        b = something_else(make(103, 41, "rk2")).load_session(path)
        assert b.time == a.time
        for dt in dts[3:]:
            a.substep(float(dt)); b.substep(float(dt))
        assert differing(state(a), state(b)) == []
        a.close(); b.close()


# ----------------------------------------------------------------------------- 3. off in the file: off afterwards
def test_a_plain_session_switches_every_extra_off(tmp_path):
    path, snap = str(tmp_path / "plain.session"), str(tmp_path / "plain.snap")
    a = waterfall(make(100, 40))
    for _ in range(5):
        a.step()
    a.save_session(path); a.save_state(snap)
    b = something_else(make(100, 40)).load_session(path)
    c = make(100, 40).load_state(snap)
    assert b.n_tracers == 0 and len(b.bodies()[0]) == 0 and int(b.reseed()[0]["thin_above"]) == 0 and b.forcing()[0].tobytes() == ea.forcing_default().tobytes()
    assert code_of(lambda: b.heat())[0] == su.ESTATE      # heat is off
    c.time = b.time      # (the one thing a snapshot leaves to the caller)
    for _ in range(5):
        b.step(); c.step()
    assert differing(state(b, heat=False, events=False), state(c, heat=False, events=False)) == []
    for s in (a, b, c):
        s.close()


# ----------------------------------------------------------------------------- 4. no switch-on side effects
def test_the_restore_has_no_switch_on_side_effects(saved):
    path, at_save = saved
    f = ea.read_session(path, verify=False)
    b = something_else(make(100, 40)).load_session(path)
    assert b.stats().n_markers == f["n_markers"] == len(f["markers"])      # no body deleted water
    assert b.get(ea.F_SOLID).tobytes() == f["solid"].tobytes() and b.get(ea.F_MARKERS).tobytes() == f["markers"].tobytes()
    assert b.reseed()[1].tobytes() == f["reseed"]["stats"].tobytes() and int(f["reseed"]["stats"]["removed"][0]) >= 24      # the saved totals, not zero
    assert b.time == f["time"] and f["time"] > 0.59
    assert b.tracers().tobytes() == f["tracers"].tobytes() and len(f["tracers"]) == 40 and b.temperature.tobytes() == f["heat"]["field"].tobytes()
    bodies, now = b.bodies()
    assert bodies.tobytes() == f["bodies"]["bodies"].tobytes() and np.array_equal(np.stack([now["ox"], now["oy"]], 1), f["bodies"]["origins"])
    assert differing(state(b), at_save) == []
    # what the file says about the saving handle: its settings, and the counters of the frame it was saved behind
    assert int(f["settings"]["dot_mode"][0]) == ea.DOT_SEQUENTIAL and int(f["settings"]["opt"][0][ea.OPT_P_STEPS]) == 8 and f["frames"] == 6 and f["stats"]["last_substeps"] >= 1
    b.close()


# ----------------------------------------------------------------------------- 5. refusals leave the handle alone
def test_refused_loads_leave_the_handle_alone(tmp_path, saved):
    path, _ = saved
    f = ea.read_session(path, verify=False)
    good = open(path, "rb").read()

    def written(name, st=None, raw=None, chunks=None):
        p = str(tmp_path / name)
        if raw is not None:
            open(p, "wb").write(raw)
        else:
            ea.write_session(p, st, chunks)
        return p

    flipped = bytearray(good); flipped[len(good) // 3] ^= 0x20
    pay = ea.session_payloads(f)
    chunks = [(t, 1, p) for t, p in zip(ea.SESSION_TAGS, pay)]
    sett = dict(f, settings=f["settings"].copy())
    sett["settings"]["max_substeps"] = 4
    opened = dict(f, solid=f["solid"].copy())
    ox, oy = f["bodies"]["origins"][0]
    opened["solid"][oy, ox] = 0
    hot = dict(f, heat=dict(f["heat"], field=f["heat"]["field"].copy()))
    hot["heat"]["field"][20, 30] = 20000.0
    sett_path = written("sett", sett)
    cases = [("wrong X", written("x", dict(f, X=101)), su.EINVAL, "101x40"), ("a corrupted byte", written("flip", raw=bytes(flipped)), su.EIO, "checksum"),
             ("truncated", written("short", raw=good[: len(good) * 2 // 3]), su.EIO, ""), ("an unknown tag", written("tag", f, chunks=chunks[:4] + [(b"WIND", 1, b"")] + chunks[4:]), su.EINVAL, "WIND"),
             ("a settings mismatch", sett_path, su.ESTATE, "max_substeps"), ("a body over an open cell", written("body", opened), su.EINVAL, "open"),
             ("a heat value beyond 1e4", written("hot", hot), su.EINVAL, "1e4"), ("no such file", str(tmp_path / "none"), su.EIO, "")]
    a, twin = something_else(make(100, 40)), something_else(make(100, 40))
    for what, p, code, word in cases:
        got, msg = code_of(lambda: a.load_session(p))
        assert got == code and word in msg, (what, got, msg)
    assert a.L.euler_load_session(a.h, os.fsencode(path), 2) == su.EINVAL      # an unknown flag bit
    assert a.L.euler_load_session(None, os.fsencode(path), 0) == su.EINVAL and a.L.euler_save_session(a.h, None) == su.EINVAL
    assert differing(state(a), state(twin)) == []
    for _ in range(3):
        a.step(); twin.step()
    assert differing(state(a), state(twin)) == []
    # the settings are compared and nothing else is skipped: the same file loads with the flag, and then holds the file's state
    a.load_session(sett_path, ignore_settings=True)
    assert a.time == f["time"] and a.n_tracers == 40
    # a handle with nothing loaded has nothing to save; a slab handle refuses both calls
    empty = make(100, 40)
    assert code_of(lambda: empty.save_session(str(tmp_path / "empty")))[0] == su.ESTATE
    slab = ea.Simulation(100, 40, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, slab=(0, 1))
    for fn in (lambda: slab.save_session(str(tmp_path / "slab")), lambda: slab.load_session(path)):
        got, msg = code_of(fn)
        assert got == su.ESTATE and "slab" in msg, (got, msg)
    for s in (a, twin, empty, slab):
        s.close()


# ----------------------------------------------------------------------------- 6. euler_load_state on a session file
def test_load_state_takes_the_core_of_a_session(tmp_path):
    path, snap = str(tmp_path / "s.session"), str(tmp_path / "s.snap")
    a = everything(make(100, 40))
    for _ in range(6):
        a.step()
    a.save_session(path); a.save_state(snap)
    b, c = something_else(make(100, 40)).load_state(path), something_else(make(100, 40)).load_state(snap)
    assert b.time == 0.0 and b.n_tracers == 0 and len(b.bodies()[0]) == 0 and (b.temperature == F32(3.0)).all()      # the extras by the rules of a snapshot
    assert differing(state(b), state(c)) == []
    for _ in range(3):
        b.step(); c.step()
    assert differing(state(b), state(c)) == []
    flipped = bytearray(open(path, "rb").read()); flipped[-40] ^= 1      # a byte of the chunks: the checksum covers them
    open(path + ".bad", "wb").write(bytes(flipped))
    assert code_of(lambda: b.load_state(path + ".bad"))[0] == su.EIO
    for s in (a, b, c):
        s.close()


def test_two_slabs_load_a_session_as_they_load_the_snapshot(tmp_path):
    X, Y = 200, 330
    path, snap = str(tmp_path / "whole.session"), str(tmp_path / "whole.snap")
    whole = waterfall(ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE))
    whole.add_tracers(np.array([[5.5, 300.5]], F32)).set_forcing(gravity=(1.0, -10.0))
    for _ in range(8):
        whole.step()
    whole.save_session(path); whole.save_state(snap)
    whole.close()
    rc, out, err = ranks.launch(2, os.path.join(ROOT, "tests", "session_slab_worker.py"), [X, Y, snap, path], 29741, timeout=600)
    assert rc == 0, (out[-1500:], err[-4000:])
    d = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert d["differ"] == [] and d["differ_after_a_frame"] == [] and d["markers"] > 0 and d["world"] == 2, d


# ----------------------------------------------------------------------------- 7. versions 1 and 2 unchanged
@pytest.mark.parametrize("rainbow", [False, True])
def test_save_state_still_writes_versions_1_and_2(tmp_path, rainbow):
    a = everything(make(100, 40, "rainbow" if rainbow else "plain"))
    for _ in range(4):
        a.step()
    p, q = str(tmp_path / "a.snap"), str(tmp_path / "b.snap")
    a.save_state(p)
    st = {n: a.get(f) for n, f in FIELDS + (DYE if rainbow else ())}
    t = a.stats()
    st.update(rng_state=t.rng_state, source_exhausted=t.source_exhausted, frames=t.frames, total_substeps=t.total_substeps, total_pcg_iterations=t.total_pcg_iterations)
    st["markers"] = st["markers"].reshape(-1, 2)
    ea.write_snapshot(q, st)
    raw = open(p, "rb").read()
    assert raw == open(q, "rb").read() and struct.unpack_from("<I", raw, 8)[0] == (2 if rainbow else 1)
    a.close()


# ----------------------------------------------------------------------------- 8. the command line
EXTRAS = ["--gravity", "1.5,-9.5", "--shake", "2,0.5:0.5:20", "--force", "3,0.5:60,2,67,6", "--heat", "0:0.5:0.3", "--heat-source", "8", "--heat-box", "fix:16:2,30,12,34",
          "--body", "3,2:8,32:0,0:3,0:0.5", "--reseed", "16:fill", "--tracer-box", "3,33,10,36:1", "--tracer", "30.5,2.5"]
OBSERVERS = ["--emit", "12.5,30.5:2", "--emit", "5.5,20.5:3", "--edit", "8:solid:30,20,33,22", "--edit", "3:fill:40,5,48,9", "--gauge", "level:1,1,98,38", "--gauge", "flux:20,1,20,38"]


def cli(tmp_path, tag, args, keys=None):
    files = {k: str(tmp_path / ("%s.%s.csv" % (tag, k))) for k in ("stats", "gauges", "tracers")}
    cmd = [EXE, "--dump", "--no-pace"] + args + ["--stats", files["stats"], "--tracers", files["tracers"]] + (["--gauges", files["gauges"]] if "--gauge" in args else [])
    cmd += ["--keys", keys] if keys else []
    r = subprocess.run(cmd, capture_output=True, timeout=300)
    return r, {k: open(v).read().splitlines() if os.path.exists(v) else [] for k, v in files.items()}


def from_frame(lines, f0):
    return [l for l in lines[1:] if int(l.split(",")[0]) >= f0]


def test_the_command_line_resumes_where_it_stopped(tmp_path):
    scen = str(tmp_path / "waterfall.txt")
    open(scen, "w").write(scenarios.waterfall())
    sess = str(tmp_path / "s.session")
    whole, wf = cli(tmp_path, "whole", ["--frames", "12"] + EXTRAS + OBSERVERS + [scen])
    first, _ = cli(tmp_path, "first", ["--frames", "6", "--session-out", sess] + EXTRAS + OBSERVERS + [scen])
    second, sf = cli(tmp_path, "second", ["--frames", "12", "--session-in", sess] + OBSERVERS)
    assert whole.returncode == 0 and first.returncode == 0 and second.returncode == 0, (whole.stderr[-800:], first.stderr[-800:], second.stderr[-800:])
    mark = b"--- frame 6 "
    assert second.stdout.startswith(mark) and whole.stdout.count(mark) == 1
    assert second.stdout == whole.stdout[whole.stdout.index(mark):]
    assert first.stdout == whole.stdout[: whole.stdout.index(b"--- frame 7 ")]
    for k in ("stats", "gauges", "tracers"):
        assert wf[k][0] == sf[k][0] and from_frame(sf[k], 0) == from_frame(wf[k], 6) and len(from_frame(sf[k], 0)) >= 7, k
    # the edit of frame 8 and the emitters' schedule landed on the same frames: the tracer count per frame is the uninterrupted run's
    per_frame = lambda lines: [sum(1 for l in lines[1:] if int(l.split(",")[0]) == f) for f in range(6, 13)]
    assert per_frame(sf["tracers"]) == per_frame(wf["tracers"]) and per_frame(sf["tracers"])[-1] > per_frame(sf["tracers"])[0]
    # --session-every leaves a loadable file behind an early q: written behind frame 3, and again at the exit, behind frame 4
    early = str(tmp_path / "early.session")
    r, _ = cli(tmp_path, "early", ["--frames", "12", "--session-out", early, "--session-every", "3"] + EXTRAS + [scen], keys="....q")
    assert r.returncode == 0 and ea.read_session(early)["frames"] == 4 and not os.path.exists(early + ".tmp")
    r, _ = cli(tmp_path, "late", ["--frames", "5", "--session-in", early])
    assert r.returncode == 0 and r.stdout.startswith(b"--- frame 4 ") and r.stdout.count(b"--- frame ") == 2
    # what the file carries cannot be given again; a setting that differs names its field
    for bad in (["--resume", sess], ["--upscale"], ["--gravity", "0,-5"], ["--shake", "1,0:1"], ["--force", "1,1:2,2,5,5"], ["--heat", "0:0.5"], ["--heat-source", "3"],
                ["--body", "2,2:8,8:0,0"], ["--reseed", "16"], ["--tracer", "5.5,5.5"], ["--tracer-box", "3,3,5,5:1"], [scen]):
        r = subprocess.run([EXE, "--dump", "--frames", "7", "--session-in", sess] + bad, capture_output=True, timeout=120)
        assert r.returncode == 1 and b"usage" in r.stderr, (bad, r.stderr[-300:])
    r = subprocess.run([EXE, "--dump", "--frames", "7", "--session-in", sess, "--advection", "rk2"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"option 22" in r.stderr, r.stderr[-300:]
    r = subprocess.run([EXE, "--dump", "--frames", "3", "--session-every", "2", scen], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"usage" in r.stderr


def test_a_run_without_the_new_flags_and_checkpoint_resume_are_unchanged(tmp_path):
    """--checkpoint still writes the bytes of euler_save_state (version 1) and --resume still starts at frame 0 from them with the extras given again"""
    scen = str(tmp_path / "waterfall.txt")
    open(scen, "w").write(scenarios.waterfall())
    snap = str(tmp_path / "c.snap")
    r = subprocess.run([EXE, "--dump", "--frames", "4", "--checkpoint", snap, scen], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(b"--- frame ") == 5
    a = waterfall(make(100, 40))
    for _ in range(4):
        a.step()
    a.save_state(snap + ".lib")
    assert open(snap, "rb").read() == open(snap + ".lib", "rb").read() and ea.read_snapshot(snap)["frames"] == 4
    r2 = subprocess.run([EXE, "--dump", "--frames", "2", "--resume", snap], capture_output=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout.startswith(b"--- frame 0 ") and r2.stdout.count(b"--- frame ") == 3
    frames = lambda out: [c.split(b"\n", 1)[1] for c in out.split(b"--- frame ")[1:]]
    assert frames(r2.stdout)[0] == frames(r.stdout)[4]
    a.close()
