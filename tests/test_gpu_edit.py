"""euler_edit_box on the GPU (docs/editing.md) against its numpy restatement (tests/edit_ref.py) and the oracle: the edit itself, the continuation from the edited
state, the device edit against a load of the host-edited snapshot in every solver / advection mode, the lean stage forms, the observers right after an edit, the
refusals and the source bookkeeping.  Grids 96 x 64, 101 x 45 (ragged: X % 4 != 0) and 130 x 70 (tile boundaries in x and y): six hand-placed boxes of at most 22 x 21 cells, at most 12 k markers.
Boxes of several workgroups, every edge alignment, markers on a box's edges and the paths only millions of markers or cells reach: test_gpu_edit_boxes.py."""
import numpy as np
import pytest

import diagnostics_ref as dref
import edit_ref as er
import euler_amd as ea
import viewport_ref as vref
import overview_ref as oref
from euler_amd import scenarios
from golden_util import load, scenario_text
from observer_util import DYE, EULER_EINVAL, EULER_ESTATE
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

GRID_FIELDS = {"solid": ea.F_SOLID, "source": ea.F_SOURCE, "sink": ea.F_SINK, "count": ea.F_COUNT, "prev_count": ea.F_PREV_COUNT, "u": ea.F_U, "v": ea.F_V,
               "utmp": ea.F_UTMP, "vtmp": ea.F_VTMP, "precon": ea.F_PRECON}
EDITED = ("solid", "source", "sink", "count", "prev_count", "u", "v")      # what the edit itself is compared on, besides the markers, n and the RNG
RUN_FIELDS = (ea.F_U, ea.F_V, ea.F_COUNT, ea.F_PREV_COUNT, ea.F_MARKERS, ea.F_PRECON, ea.F_SOLID, ea.F_SOURCE, ea.F_SINK)
ALL_OPS = list(er.BOXES_96x64)


def read_state(sim):
    st = {n: sim.get(f) for n, f in GRID_FIELDS.items()}
    s = sim.stats()
    st.update(markers=sim.get(ea.F_MARKERS), rng_state=int(s.rng_state), source_exhausted=int(s.source_exhausted), X=sim.X, Y=sim.Y)
    assert len(st["markers"]) == s.n_markers
    return st


def load_state(sim, state):
    for n, f in GRID_FIELDS.items():
        sim.set(f, state[n])
    sim.set_markers(state["markers"])
    sim.set_rng(state["rng_state"], state["source_exhausted"])
    return sim


def assert_state(sim, want, what, fields=EDITED):
    got = read_state(sim)
    for n in fields:
        assert_bits(got[n], np.asarray(want[n]), "%s %s" % (what, n))
    assert len(got["markers"]) == len(want["markers"]), (what, len(got["markers"]), len(want["markers"]))
    assert_bits(got["markers"], np.asarray(want["markers"], np.float32).reshape(-1, 2), what + " markers")
    assert got["rng_state"] == want["rng_state"] and got["source_exhausted"] == want["source_exhausted"], what


def apply(sim, grid, what):
    for name in er.SEQUENCE if what == "sequence" else (what,):
        sim.edit_box(er.OPS[name], er.scaled_box(name, *grid))


def dam_break(grid, frames=er.FRAMES_BEFORE, options=(), **kw):
    sim = ea.Simulation(grid[0], grid[1], **kw)
    for k, v in options:
        sim.set_option(k, v)
    sim.load_text(scenarios.dam_break(), upscale=True)
    for _ in range(frames):
        sim.step()
    return sim


# ----------------------------------------------------------------------------- 1. the edit itself
@pytest.mark.parametrize("grid", er.GRIDS)
def test_each_op_and_the_sequence_equal_the_restatement(grid):
    """after 4 frames of the handle's own run: every op alone on a fresh copy of that state, then the six in sequence on one handle - compared after every op"""
    sim = dam_break(grid, dot_mode=ea.DOT_SEQUENTIAL)
    start = read_state(sim)
    assert_state(sim, er.base_state(*grid), "the run before the edit")      # (the oracle's state: what tests 2 and 3 start from)
    before = sim.hbm_bytes()
    for name in ALL_OPS:
        box = er.scaled_box(name, *grid)
        h = load_state(ea.Simulation(grid[0], grid[1], dot_mode=ea.DOT_SEQUENTIAL), start)
        h.edit_box(er.OPS[name], box)
        want = er.edit_state(start, er.OPS[name], box)
        print("%s %s box %s: %d -> %d markers" % (grid, name, box, len(start["markers"]), len(want["markers"])))
        assert_state(h, want, "%s alone" % name, fields=tuple(GRID_FIELDS))
        assert_state(h, er.edited_state(grid[0], grid[1], name), "%s alone, the shared restatement" % name)
        h.close()
    st = start
    for name in er.SEQUENCE:
        box = er.scaled_box(name, *grid)
        sim.edit_box(er.OPS[name], box)
        st = er.edit_state(st, er.OPS[name], box)
        assert_state(sim, st, "sequence, after %s" % name, fields=tuple(GRID_FIELDS))
    assert sim.hbm_bytes() == before      # the edit works in the marker stage's scratch
    sim.close()


@pytest.mark.parametrize("grid", er.GRIDS)
def test_edit_between_two_substeps_of_one_frame(grid):
    """frame 12 of the dam break takes several substeps: every op between its first two, then the second against the oracle from the restated state"""
    sim = dam_break(grid, frames=14, dot_mode=ea.DOT_SEQUENTIAL)
    dt = sim.timestep(0.1)
    assert 0 < dt < 0.1      # (a frame of more than one substep)
    sim.substep(dt)
    mid = read_state(sim)
    for name in ALL_OPS:
        box = er.scaled_box(name, *grid)
        h = load_state(ea.Simulation(grid[0], grid[1], dot_mode=ea.DOT_SEQUENTIAL), mid) if name != ALL_OPS[-1] else sim      # (the last op on the running handle itself)
        h.edit_box(er.OPS[name], box)
        want = er.edit_state(mid, er.OPS[name], box)
        assert_state(h, want, "%s between substeps" % name, fields=tuple(GRID_FIELDS))
        o = er.parity_oracle(want)
        dt2 = o.timestep(0.1 - dt)
        assert h.timestep(0.1 - dt) == dt2
        it = o.substep(dt2)
        h.substep(dt2)
        assert h.stats().last_pcg_iterations == it
        for f in ("u", "v", "count", "prev_count"):
            assert_bits(h.get(GRID_FIELDS[f]), np.array(getattr(o, f)), "%s, the next substep: %s" % (name, f))
        assert_bits(h.get(ea.F_MARKERS), np.array(o.markers), "%s, the next substep: markers" % name)
        o.close()
        h.close()


# ----------------------------------------------------------------------------- 2. continuation against the oracle
@pytest.mark.parametrize("what", ALL_OPS + ["sequence"])
@pytest.mark.parametrize("grid", er.GRIDS)
def test_continuation_equals_the_oracle(grid, what):
    """parity mode, sequential dots: the handle edited on the device and the oracle from the restated state, 25 frames, every frame"""
    sim = load_state(ea.Simulation(grid[0], grid[1], dot_mode=ea.DOT_SEQUENTIAL), er.base_state(*grid))
    apply(sim, grid, what)
    assert_state(sim, er.edited_state(grid[0], grid[1], what), "edited")
    iters = 0
    for f, rec in enumerate(er.continued(grid[0], grid[1], what)):
        sim.step()
        s = sim.stats()
        assert (s.last_substeps, s.last_pcg_iterations) == (rec["substeps"], rec["iterations"]), (f, s.last_substeps, s.last_pcg_iterations, rec["substeps"], rec["iterations"])
        iters += s.last_pcg_iterations
        for n in ("u", "v", "count", "prev_count", "solid", "source", "sink"):
            assert_bits(sim.get(GRID_FIELDS[n]), rec[n], "%s frame %d %s" % (what, f, n))
        assert_bits(sim.get(ea.F_MARKERS), rec["markers"], "%s frame %d markers" % (what, f))
        assert s.rng_state == rec["rng_state"], f
    assert iters > 1000
    sim.close()


# ----------------------------------------------------------------------------- 3. device edit = load of the host-edited snapshot
MODES = {
    "parity": ((130, 70), dict(dot_mode=ea.DOT_SEQUENTIAL), ()),
    "tile_resident": ((96, 64), dict(precond=ea.PRECOND_IC0_TILE, dot_mode=ea.DOT_TREE), ()),
    "tile_resident_off": ((101, 45), dict(precond=ea.PRECOND_IC0_TILE, dot_mode=ea.DOT_TREE, resident=ea.RESIDENT_OFF), ()),
    "multilevel_uncapped": ((130, 70), dict(precond=ea.PRECOND_IC0_TILE_MG, max_iterations=2000), ()),
    "rk2_maccormack": ((101, 45), dict(dot_mode=ea.DOT_SEQUENTIAL), ((ea.OPT_ADVECT_RK2, 1), (ea.OPT_ADVECT_MACCORMACK, 1))),
    "rainbow": ((96, 64), dict(dot_mode=ea.DOT_SEQUENTIAL, rainbow=True), ()),
}
DYE_ALL = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B, ea.F_DYE_RTMP, ea.F_DYE_GTMP, ea.F_DYE_BTMP)


def same_run(a, b, fields, frames, what):
    for f in range(frames):
        a.step(); b.step()
        if f % 6 == 0 or f == frames - 1:
            for fld in fields:
                assert_bits(b.get(fld), a.get(fld), "%s frame %d field %d" % (what, f, fld))
    sa, sb = a.stats(), b.stats()
    assert (sa.total_substeps, sa.total_pcg_iterations, sa.n_markers, sa.rng_state) == (sb.total_substeps, sb.total_pcg_iterations, sb.n_markers, sb.rng_state), what
    return sa


@pytest.mark.parametrize("mode", list(MODES))
def test_device_edit_equals_load_of_host_edited_snapshot(mode, tmp_path):
    """Handle A edits on the device; handle B saves, has its snapshot edited by the restatement, and loads; 25 frames, bit for bit.  First the unedited control of
    the mode: continuing against save -> load -> continuing."""
    grid, kw, options = MODES[mode]
    fields = RUN_FIELDS + (DYE_ALL if kw.get("rainbow") else ())
    make = lambda: dam_break(grid, options=options, **kw)
    path = str(tmp_path / "state.snap")
    # control
    a, b = make(), make()
    b.save_state(path)
    b.load_state(path)
    same_run(a, b, fields, er.FRAMES_AFTER, mode + " control")
    a.close(); b.close()
    # the six ops in sequence
    a, b = make(), make()
    apply(a, grid, "sequence")
    b.save_state(path)
    snap = ea.read_snapshot(path)
    for name in er.SEQUENCE:
        snap = er.edit_state(snap, er.OPS[name], er.scaled_box(name, *grid))
    ea.write_snapshot(path, snap)
    b.load_state(path)
    for fld in fields:
        assert_bits(a.get(fld), b.get(fld), "%s edited, field %d" % (mode, fld))
    s = same_run(a, b, fields, er.FRAMES_AFTER, mode)
    assert s.total_pcg_iterations > 1000
    a.close(); b.close()


# ----------------------------------------------------------------------------- 4. the lean stage forms
LEAN_OFF = (ea.OPT_NO_TILE_MAP, ea.OPT_MARKERS_TWO_PASS, ea.OPT_BUILD_TWO_PASS, ea.OPT_VELOCITY_TWO_PASS, ea.OPT_MARKERS_ROWMAJOR)


@pytest.mark.parametrize("grid,kw", [((130, 70), dict(dot_mode=ea.DOT_SEQUENTIAL)), ((96, 64), dict(precond=ea.PRECOND_IC0_TILE, dot_mode=ea.DOT_TREE, resident=ea.RESIDENT_OFF)),
                                     ((101, 45), dict(precond=ea.PRECOND_IC0_TILE, dot_mode=ea.DOT_TREE))])
def test_lean_forms_give_the_bits_of_the_plain_forms(grid, kw):
    """the same edited run with the tile map, the fused marker pass, the one-pass assembly and velocity update and the column-major marker stage switched off: whatever the
    lean forms keep from one stage for the next, the edit has invalidated"""
    a = dam_break(grid, **kw)
    b = dam_break(grid, options=[(k, 1) for k in LEAN_OFF], **kw)
    apply(a, grid, "sequence"); apply(b, grid, "sequence")
    s = same_run(a, b, RUN_FIELDS, er.FRAMES_AFTER, "lean forms %s" % (grid,))
    assert s.total_pcg_iterations > 1000
    # ... and an edit in the middle of a substep's stages, behind the stage that prepared the most for the next ones
    dt = a.timestep(0.1)
    assert b.timestep(0.1) == dt
    for st in range(6):
        a.stage(st, dt); b.stage(st, dt)
        name = er.SEQUENCE[st]
        a.edit_box(er.OPS[name], er.scaled_box(name, *grid)); b.edit_box(er.OPS[name], er.scaled_box(name, *grid))
    same_run(a, b, RUN_FIELDS, 6, "lean forms %s, edits between stages" % (grid,))
    a.close(); b.close()


# ----------------------------------------------------------------------------- 5. the observers see the edit
@pytest.mark.parametrize("grid", er.GRIDS)
def test_observers_see_the_edit(grid):
    """right after FILL (96 x 64, 101 x 45: into a tile without water) and after SOLID: euler_diagnostics, euler_overview_box and euler_marker_raster equal their numpy
    restatements on the restated state - the tile map they were reading before the edit no longer counts"""
    sim = dam_break(grid, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True)
    whole = (1, 1, grid[0] - 2, grid[1] - 2)
    st = read_state(sim)
    dye = tuple(sim.get(f) for f in DYE)
    for name in ("fill", "solid"):
        box = er.scaled_box(name, *grid)
        sim.diagnostics_record(whole); sim.overview(7, 5); sim.marker_raster(box, 2)      # (the passes have run on the state before)
        sim.edit_box(er.OPS[name], box)
        st = er.edit_state(st, er.OPS[name], box)
        for b in (whole, box):
            bw, bh = b[2] - b[0] + 1, b[3] - b[1] + 1
            assert not dref.mismatches(sim.diagnostics_record(b), dref.diag_ref(st["solid"], st["count"], st["u"], st["v"], b)), (name, b)
            for w, h in ((bw, bh), (max(1, bw // 3), max(1, bh // 2))):
                bad = oref.mismatches(sim.overview(w, h, box=b), vref.overview_box_ref(st["solid"], st["sink"], st["count"], st["u"], st["v"], dye, b, w, h))
                assert not bad, (name, b, w, h, bad)
            assert np.array_equal(sim.marker_raster(b, 2), vref.raster_ref(st["markers"], b, 2)), (name, b)
        if name == "fill" and grid != (130, 70):      # every cell of the box was dry: four markers each show
            assert sim.diagnostics(box)["markers"] == 4 * (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
    sim.close()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals():
    X, Y = 96, 64
    L = ea.load_library()
    assert L.euler_edit_box(None, ea.EDIT_FILL, 1, 1, 2, 2) == EULER_EINVAL
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:
        slab.edit_box(ea.EDIT_FILL, (1, 1, 2, 2))
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    with pytest.raises(ea.EulerError) as e:      # (the slab refusal comes before the box check)
        slab.edit_box(99, (0, 0, 0, 0))
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL)
    for args in ((ea.EDIT_FILL, (1, 1, 2, 2)), (99, (0, 0, 0, 0))):      # nothing loaded: before the box and op checks
        with pytest.raises(ea.EulerError) as e:
            sim.edit_box(*args)
        assert e.value.code == EULER_ESTATE
    sim.load_text(scenarios.dam_break(), upscale=True)
    for _ in range(3):
        sim.step()
    start = read_state(sim)
    hbm = sim.hbm_bytes()
    bad_boxes = ((0, 1, 10, 10), (1, 0, 10, 10), (1, 1, X - 1, 10), (1, 1, 10, Y - 1), (11, 1, 10, 10), (1, 11, 10, 10), (-5, -5, -1, -1))
    for op in range(6):
        for box in bad_boxes:
            with pytest.raises(ea.EulerError) as e:
                sim.edit_box(op, box)
            assert e.value.code == EULER_EINVAL, (op, box)
    for op in (-1, 6, 100):
        with pytest.raises(ea.EulerError) as e:
            sim.edit_box(op, (5, 5, 9, 9))
        assert e.value.code == EULER_EINVAL, op
    assert_state(sim, start, "after the refusals", fields=tuple(GRID_FIELDS))
    assert sim.hbm_bytes() == hbm
    # capacity: 4 X Y - 10 markers piled into a few cells, then FILL (or SOURCE) an empty box of 16 x 11 cells
    pile = np.tile(np.array([[50.25, 50.75], [50.75, 51.25], [51.5, 50.5]], np.float32), (4 * X * Y, 1))[: 4 * X * Y - 10]
    sim.set_markers(pile)
    full = read_state(sim)
    for op in (ea.EDIT_FILL, ea.EDIT_SOURCE):
        with pytest.raises(ea.EulerError) as e:
            sim.edit_box(op, er.scaled_box("fill", X, Y))
        assert e.value.code == EULER_EINVAL
        assert_state(sim, full, "after the capacity refusal", fields=tuple(GRID_FIELDS))
    assert sim.hbm_bytes() == hbm
    sim.edit_box(ea.EDIT_FILL, (70, 40, 71, 40))      # two cells still fit: n + 8 = 4 X Y - 2 <= 4 X Y - 1
    assert_state(sim, er.edit_state(full, ea.EDIT_FILL, (70, 40, 71, 40)), "the last two cells", fields=tuple(GRID_FIELDS))
    with pytest.raises(ea.EulerError) as e:
        sim.edit_box(ea.EDIT_FILL, (72, 40, 72, 40))      # n + 4 = 4 X Y + 2
    assert e.value.code == EULER_EINVAL
    sim.close()


# ----------------------------------------------------------------------------- 7. source bookkeeping
def test_clear_over_the_waterfalls_sources_stops_the_appends():
    g = load("waterfall_frames.npz")
    text = scenario_text(g)
    X, Y = g["solid"].shape[1], g["solid"].shape[0]
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(text)
    n = [sim.stats().n_markers]
    for _ in range(6):
        sim.step()
        n.append(sim.stats().n_markers)
    assert n[-1] > n[0]      # it pours
    st = read_state(sim)
    ys, xs = np.nonzero(st["source"])
    box = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
    hbm = sim.hbm_bytes()
    sim.edit_box(ea.EDIT_CLEAR, box)
    assert sim.hbm_bytes() == hbm      # no new buffer
    st = er.edit_state(st, ea.EDIT_CLEAR, box)
    assert not st["source"].any()
    assert_state(sim, st, "cleared", fields=tuple(GRID_FIELDS))
    o = er.parity_oracle(st)
    for f in range(8):
        o.step(); sim.step()
        s = sim.stats()
        assert s.n_markers <= n[-1] and s.rng_state == st["rng_state"], f      # no append, no draw
        assert_bits(sim.get(ea.F_MARKERS), np.array(o.markers), "frame %d markers" % f)
        assert_bits(sim.get(ea.F_U), np.array(o.u), "frame %d u" % f)
        assert_bits(sim.get(ea.F_COUNT), np.array(o.count), "frame %d count" % f)
    # ... and SOURCE over a part of them starts it again, as the oracle's
    part = (box[0], box[1], box[0] + 3, box[3])
    st = read_state(sim)
    hbm = sim.hbm_bytes()
    sim.edit_box(ea.EDIT_SOURCE, part)
    assert sim.hbm_bytes() == hbm
    st = er.edit_state(st, ea.EDIT_SOURCE, part)
    assert_state(sim, st, "sources again", fields=tuple(GRID_FIELDS))
    o.close()
    o = er.parity_oracle(st)
    grew = False
    for f in range(6):
        before = sim.stats().n_markers
        o.step(); sim.step()
        grew = grew or sim.stats().n_markers > before
        assert_bits(sim.get(ea.F_MARKERS), np.array(o.markers), "frame %d markers" % f)
        assert sim.stats().rng_state == int(o.c.rng_state)
    assert grew
    o.close(); sim.close()
