"""euler_set_reseed on the GPU (docs/reseed.md): the marker density control against the test-side restatement (tests/reseed_ref.py, pinned on the CPU by
test_reseed_host.py), bit for bit in the parity mode: one pass teacher-forced on planted states (crowded cells at tile corners and next to the border, markers on
sub-cell boundaries, duplicates, a wrapped count byte, the limits, deletions in the tail, the array's capacity, the eight-neighbour rule against a hand-written
table), free runs under each transport, with the dye, a forcing and the temperature, in the lean and the full forms of the stages, the properties (off: no trace;
nothing to do: nothing done; the diagnostics agree; the bound holds in the other solver modes), the refusals and `euler --reseed`.
Grids 96 x 64, 101 x 45 (X % 4 != 0: one cell per lane, a ragged last mask word) and 130 x 70 (tiles of the tile map both ways)."""
import functools
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import edit_ref as eref
import euler_amd as ea
import forcing_ref as fref
import heat_ref as href
import reseed_ref as rref
from euler_amd import scenarios
from observer_util import EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames
from oracle_lib import Oracle
from resident_ref import oracle_from_state
from test_gpu_edit import load_state
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

GRIDS = [(96, 64), (101, 45), (130, 70)]
F32 = np.float32
MASKS = ((ea.F_SOLID, "solid"), (ea.F_SOURCE, "source"), (ea.F_SINK, "sink"), (ea.F_COUNT, "count"), (ea.F_PREV_COUNT, "prev_count"))
LEAN_OFF = ((ea.OPT_NO_TILE_MAP, 1), (ea.OPT_MARKERS_TWO_PASS, 1), (ea.OPT_MARKERS_ROWMAJOR, 1))


_AM = {}      # the transports' library of the module's fixture, for the cached reference runs


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    _AM["lib"] = amref.build(tmp_path_factory.mktemp("reseed_gpu"))
    return _AM["lib"]


def record(r):
    return ea.reseed(r["thin_above"], r["fill_holes"], r["max_cells"], r["max_fill"])


def totals(sim):
    st = sim.reseed()[1]
    return {k: int(st[k]) for k in rref.STAT_NAMES}


def compare(sim, o, what, stats=None):
    for fld, n in MASKS:
        assert_bits(sim.get(fld), getattr(o, n), "%s %s" % (what, n))
    s = sim.stats()
    assert s.n_markers == o.n_markers, (what, s.n_markers, o.n_markers)
    assert_bits(sim.get(ea.F_MARKERS), o.markers, what + " markers")
    assert (s.rng_state, s.source_exhausted) == (int(o.c.rng_state), int(o.c.source_exhausted)), what
    if stats is not None:
        assert totals(sim) == stats, (what, totals(sim), stats)


# ----------------------------------------------------------------------------- planted states
LAB = (10, 8, 30, 22)      # a rectangle without masks, one marker in the middle of every cell but the ones HOLE_TABLE empties; it fits every grid
# cell -> (what is planted there, is it a hole?)  The eight-neighbour rule by hand: a hole has count 0, was water a refresh ago, carries no mask, and every
# neighbour is wet or solid - a sink never holds markers behind a refresh, so a sink next door always disqualifies; a source does only while it is empty.
HOLE_TABLE = {
    (13, 11): ("empty", True),
    (16, 11): ("empty, (17, 11) solid", True),
    (19, 11): ("empty, (20, 11) sink", False),
    (22, 11): ("empty, (23, 11) a source cell with a marker", True),
    (25, 11): ("empty, (26, 11) an empty source cell", False),
    (13, 15): ("empty and solid", False),
    (16, 15): ("empty and sink", False),
    (19, 15): ("empty and source", False),
    (22, 15): ("empty, dry a refresh ago too", False),
    (25, 15): ("empty, (26, 15) empty as well", False),
    (26, 15): ("empty, (25, 15) empty as well", False),
    (13, 19): ("empty", True),
    (16, 19): ("empty, (15, 18) solid", True),
    (19, 19): ("empty", True),
    (1, 12): ("empty, next to the border's sink ring", False),
}
SET_MASKS = {(17, 11): "solid", (20, 11): "sink", (23, 11): "source", (26, 11): "source", (13, 15): "solid", (16, 15): "sink", (19, 15): "source", (15, 18): "solid"}
NO_MARKER = set(HOLE_TABLE) | {(17, 11), (20, 11), (26, 11), (15, 18)}
BOUNDARY = np.array([(a, b) for a in (0.0, 0.25, 0.5, 0.75) for b in (0.0, 0.25, 0.5, 0.75)], F32)


def crowded_cells(X, Y):
    """tile corners (where the grid has them), the last column and row inside the border, the first interior cell"""
    cand = [(63, 40), (64, 40), (63, 63), (64, 63), (63, 64), (64, 64), (X - 2, 5), (40, Y - 2), (X - 2, Y - 2), (1, 1)]
    return [c for k, c in enumerate(cand) if c[0] <= X - 2 and c[1] <= Y - 2 and c not in cand[:k]]


@functools.lru_cache(maxsize=None)
def planted_state(X, Y, tail_only=False, fill_to_capacity=False):
    """edit_ref.synthetic_state (random masks, markers, velocities) with the lab, the crowded cells, the two heavy cells and the duplicates planted.  The device and
    the restatement both refresh first: count is then the bins of the markers outside sink and solid cells and prev_count the count grid loaded here.
    tail_only: the only crowded cell's markers are the last ones of the array.  fill_to_capacity: n = max_markers - 2 (the surplus sits in one far cell)."""
    rng = np.random.default_rng(X * 1000 + Y)
    st = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in eref.synthetic_state(X, Y, 40 + X, (5 * X * Y) // 4).items()}
    m = st["markers"]
    cells = crowded_cells(X, Y)
    heavy = [(35, 30), (37, 30)]      # 260 markers: the byte reads 4, the cell is left alone; 300: the byte reads 44, the cell is thinned
    x0, y0, x1, y1 = LAB
    clear = np.zeros((Y, X), bool)
    clear[y0:y1 + 1, x0:x1 + 1] = True
    clear[10:15, 1:4] = True      # the patch at the border around (1, 12)
    for cx, cy in cells + heavy:
        clear[cy, cx] = True
    for n in ("solid", "sink", "source"):
        st[n][clear] = 0
    for (cx, cy), n in SET_MASKS.items():
        st[n][cy, cx] = 1
    m = m[~clear[np.floor(m[:, 1]).astype(int), np.floor(m[:, 0]).astype(int)]]
    if tail_only or fill_to_capacity:      # the refresh deletes nothing: no marker in a sink or solid cell
        blocked = (st["solid"] != 0) | (st["sink"] != 0)
        m = m[~blocked[np.floor(m[:, 1]).astype(int), np.floor(m[:, 0]).astype(int)]]
    if tail_only:      # nothing else is crowded: at most two markers per cell elsewhere
        order = np.lexsort((np.floor(m[:, 0]), np.floor(m[:, 1])))
        cell = np.floor(m[order, 1]).astype(int) * X + np.floor(m[order, 0]).astype(int)
        rank = np.arange(len(cell)) - np.searchsorted(cell, cell)
        m = m[np.sort(order[rank < 2])]
    ys, xs = np.nonzero(clear)
    lab = np.array([(x + 0.5, y + 0.5) for x, y in zip(xs, ys) if (x, y) not in NO_MARKER and (x, y) not in cells + heavy], F32)
    planted = []
    for k, (cx, cy) in enumerate(cells):
        if (cx, cy) == (40, Y - 2):      # 20 markers in three sub-cells: the count becomes 3
            p = np.array([(0.1, 0.1), (0.6, 0.1), (0.9, 0.9)], F32)[rng.integers(0, 3, 20)] + rng.uniform(0, 0.05, (20, 2)).astype(F32)
        else:                            # every sub-cell's corner, eight anywhere, and four times one position
            p = np.concatenate([BOUNDARY, rng.uniform(0.001, 0.999, (8, 2)).astype(F32), np.full((4, 2), 0.3, F32)])
            rng.shuffle(p)
        planted.append(p + np.array([cx, cy], F32))
    h260 = rng.uniform(0.001, 0.999, (260, 2)).astype(F32) + np.array(heavy[0], F32)
    h300 = rng.uniform(0.001, 0.999, (300, 2)).astype(F32) + np.array(heavy[1], F32)
    if tail_only:
        m = np.concatenate([lab, m, h260, planted[0]])
    else:      # crowded cells in front, in the middle and - the 300 - at the very end of the array
        half = len(m) // 2
        m = np.concatenate(planted[:2] + [m[:half], lab, h260] + planted[2:] + [m[half:], h300])
    if fill_to_capacity:
        far = np.array([50.5, 30.5], F32)
        st["solid"][30, 50] = st["sink"][30, 50] = st["source"][30, 50] = 0
        m = np.concatenate([m, np.tile(far, (4 * X * Y - 2 - len(m), 1))])
    elif len(m) % 2 == 0:      # n odd - no multiple of 64 or 128: the last marker is alone in its lane, the last mask word ragged
        m = np.concatenate([np.array([(11.5, 9.5)], F32), m])      # (a second marker in a lab cell, in front of the array)
    st["markers"] = np.ascontiguousarray(m, F32)
    count = eref.bins(st["markers"], X, Y)
    for (cx, cy), (_, _) in HOLE_TABLE.items():
        count[cy, cx] = 0 if (cx, cy) == (22, 15) else 1      # water a refresh ago (but for the one that was dry), no marker now
    st["count"] = count
    st["prev_count"] = count.copy()
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


def both_passes(st, r, passes=1, **kw):
    """the refresh stage `passes` times on a handle loaded from st with the record set, and the oracle's refresh + the restated pass -> (sim, oracle, totals)"""
    sim = load_state(ea.Simulation(st["X"], st["Y"], **kw), st)
    if r is not None:
        sim.set_reseed(record(r))
    o = oracle_from_state(st)
    stats = rref.new_stats()
    for _ in range(passes):
        sim.stage(ea.STAGE_REFRESH_COUNTS)
        o.lib.eo_refresh_marker_counts(o.ptr)
        rref.apply(o, r, stats)
    return sim, o, stats


RECORDS = {"both": rref.reseed(16, True), "thin": rref.reseed(16, False), "fill": rref.reseed(0, True), "tight": rref.reseed(4, True, 3, 3)}


@pytest.mark.parametrize("which", sorted(RECORDS))
@pytest.mark.parametrize("size", GRIDS)
def test_one_pass_teacher_forced(size, which):
    X, Y = size
    st, r = planted_state(X, Y), RECORDS[which]
    assert len(st["markers"]) % 64 != 0 and len(st["markers"]) % 128 != 0
    sim, o, stats = both_passes(st, r)
    what = "%dx%d %s" % (X, Y, which)
    compare(sim, o, what, stats)
    count = np.array(o.count)
    if r["thin_above"] == 16:      # by hand: the planted cells, the wrapped bytes, the survivors
        for cx, cy in crowded_cells(X, Y):
            assert count[cy, cx] == (3 if (cx, cy) == (40, Y - 2) else 16), (cx, cy)
        assert count[30, 35] == 4 and count[30, 37] == 16      # 260 markers escape (the limit docs/reseed.md states), 300 are thinned
        assert stats["cells_thinned"] >= len(crowded_cells(X, Y)) + 1 and stats["removed"] >= 284 and stats["deferred"] == 0
    if r["fill_holes"] and which != "tight":
        for (cx, cy), (why, hole) in HOLE_TABLE.items():
            assert count[cy, cx] == (1 if hole else 0), (cx, cy, why)
        assert stats["added"] == sum(h for _, h in HOLE_TABLE.values())
        new = np.array(o.markers)[-stats["added"]:]
        assert [(int(x), int(y)) for x, y in np.floor(new)] == sorted((c for c, (_, h) in HOLE_TABLE.items() if h), key=lambda c: (c[1], c[0]))
    if which == "tight":      # three cells and three holes per pass, the rest deferred
        holes = sorted((c for c, (_, h) in HOLE_TABLE.items() if h), key=lambda c: (c[1], c[0]))
        assert stats["cells_thinned"] == 3 and stats["added"] == 3 and stats["deferred"] > len(holes) - 3
        assert [int(count[cy, cx]) for cx, cy in holes] == [1, 1, 1, 0, 0, 0]
        # A second pass takes the next three cells.  It finds no hole: the refresh in front of it has rotated the holes' zeros into prev_count - a hole is caught
        # in the substep it opens or not at all (docs/reseed.md).  With the count grid of a wet cell put back on both sides it takes the next three holes as well.
        patched = np.array(o.count)
        for cx, cy in holes[3:]:
            patched[cy, cx] = 1
        sim.set(ea.F_COUNT, patched)
        o.count[...] = patched
        for k in (2, 3):
            sim.stage(ea.STAGE_REFRESH_COUNTS)
            o.lib.eo_refresh_marker_counts(o.ptr)
            rref.apply(o, r, stats)
            compare(sim, o, "%s pass %d" % (what, k), stats)
            assert stats["cells_thinned"] == 3 * k and stats["added"] == 6
    sim.close(); o.close()


@pytest.mark.parametrize("size", GRIDS[:2])
def test_every_deleted_marker_lies_in_the_tail(size):
    st = planted_state(*size, tail_only=True)
    sim, o, stats = both_passes(st, rref.reseed(16, False))
    compare(sim, o, "tail only", stats)
    assert stats["cells_thinned"] == 1 and stats["removed"] == 28 - 16
    plain = oracle_from_state(st)      # what the refresh alone leaves (it drops the markers in sink cells): the cell's 28 markers are still the last ones
    plain.lib.eo_refresh_marker_counts(plain.ptr)
    base = np.array(plain.markers)
    assert (np.floor(base[-28:]) == np.array(crowded_cells(*size)[0], F32)).all() and len(o.markers) == len(base) - 12
    assert_bits(sim.get(ea.F_MARKERS)[: len(base) - 28], base[: len(base) - 28], "the markers in front stay where they are")
    sim.close(); o.close(); plain.close()


def test_the_array_one_short_of_full_takes_one_marker_and_leaves_the_latch():
    X, Y = 96, 64
    st = planted_state(X, Y, fill_to_capacity=True)
    assert len(st["markers"]) == 4 * X * Y - 2
    sim, o, stats = both_passes(st, rref.reseed(0, True))
    compare(sim, o, "capacity", stats)
    holes = sum(h for _, h in HOLE_TABLE.values())
    assert stats == dict(removed=0, added=1, cells_thinned=0, deferred=holes - 1)
    s = sim.stats()
    assert s.n_markers == 4 * X * Y - 1 and s.source_exhausted == 0
    sim.stage(ea.STAGE_REFRESH_COUNTS)      # the refresh has rotated the other holes' zeros into prev_count: nothing is a hole any more, and the array is full
    assert totals(sim) == dict(removed=0, added=1, cells_thinned=0, deferred=holes - 1) and sim.stats().n_markers == 4 * X * Y - 1
    sim.close(); o.close()


def launches(s):
    return {k: v[1] for k, v in s.profile().items()}


@pytest.mark.parametrize("size", GRIDS[:2])
def test_all_zero_is_a_handle_that_never_called_the_setter(size):
    st = planted_state(*size)
    a = load_state(ea.Simulation(*size), st)
    b = load_state(ea.Simulation(*size), st)
    b.set_reseed(record(rref.reseed()))
    for s in (a, b):
        s.profile_enable(ea.profile_class_names())
    for _ in range(2):
        a.stage(ea.STAGE_REFRESH_COUNTS); b.stage(ea.STAGE_REFRESH_COUNTS)
    assert launches(a) == launches(b)
    for fld in STATE_FIELDS:
        assert_bits(b.get(fld), a.get(fld), "field %d" % fld)
    assert a.stats().rng_state == b.stats().rng_state and totals(b) == rref.new_stats()
    o = oracle_from_state(st)
    for _ in range(2):
        o.lib.eo_refresh_marker_counts(o.ptr)
    compare(b, o, "off")
    a.close(); b.close(); o.close()


# ----------------------------------------------------------------------------- free runs
FREE = rref.reseed(5, True)      # seeded four to a cell, the water exceeds 5 within a few frames: the pass works in every frame of a short run


@functools.lru_cache(maxsize=None)
def _reference_run(size, scene, frames, rk2, mc, rainbow, forced, heat):
    """the composed restatement, once per configuration: per frame the grids, the markers in order and the counters -> a tuple of dicts, read-only"""
    am = _AM.get("lib")
    text = getattr(scenarios, scene)()
    o = Oracle(*size, rainbow=rainbow).load_text(text, upscale=True)
    f, boxes = (fref.forcing((3.0, -8.0), (1.5, 0.5, 0.8, 0.3)), [((10, 3, 30, 12), (4.0, -1.5))]) if forced else (None, ())
    acc_at = (lambda ff, t: ea.forcing_at(ea.forcing_record((ff["gx"], ff["gy"]), (ff["shake_x"], ff["shake_y"], ff["shake_hz"], ff["shake_phase"])), t)) if forced else None
    T = hrec = None
    if heat:
        hrec, hboxes = HEAT
        T = striped(size, hrec, np.array(o.count))
    stats, clock, out = rref.new_stats(), fref.Clock(), []
    for _ in range(frames):
        n, it = rref.step(am, o, FREE, stats, clock, f, boxes, rk2, mc, acc_at, None if not heat else (T, hrec, hboxes))
        rec = {name: np.array(getattr(o, name)) for _, name in MASKS}
        rec.update(u=np.array(o.u), v=np.array(o.v), markers=np.array(o.markers), T=None if T is None else T.copy())
        if rainbow:
            rec.update(dye=[np.array(q) for q in (o.cr, o.cg, o.cb)])
        for v in rec.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        rec.update(rng_state=int(o.c.rng_state), substeps=n, iterations=it, stats=dict(stats), time=clock.t)
        out.append(rec)
    o.close()
    return tuple(out)


HEAT = (href.heat(1.0, 0.5, 0.3), ((href.RATE, 30.0, (10, 3, 40, 12)), (href.FIX, 4.0, (25, 8, 45, 30))))


def striped(size, h, count):
    ys, xs = np.indices((size[1], size[0]))
    T = (F32(h["ambient"]) + ((xs * 3 + ys * 5) % 9).astype(F32) * F32(0.75) - F32(2.25)).astype(F32)      # something to move in every fluid cell
    T[count == 0] = F32(h["ambient"])
    return T


def free_run(am, size, scene, frames=20, rk2=0, mc=0, rainbow=False, forced=False, heat=False, options=()):
    want = _reference_run(size, scene, frames, bool(rk2), bool(mc), rainbow, forced, heat)
    sim = ea.Simulation(*size, rainbow=rainbow)
    for k, v in options:
        sim.set_option(k, v)
    sim.set_option(ea.OPT_ADVECT_RK2, rk2)
    sim.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
    sim.load_text(getattr(scenarios, scene)(), upscale=True)
    if forced:
        sim.set_forcing((3.0, -8.0), (1.5, 0.5, 0.8, 0.3), [((10, 3, 30, 12), (4.0, -1.5))])
    if heat:
        h, hboxes = HEAT
        sim.set_heat(h["ambient"], h["beta"], h["kappa"], h["source_t"], list(hboxes))
        sim.temperature = striped(size, h, sim.get(ea.F_COUNT))
    sim.set_reseed(record(FREE))
    for k, rec in enumerate(want):
        sim.step()
        what = "%dx%d %s frame %d" % (size + (scene, k))
        st = sim.stats()
        assert (st.last_substeps, st.last_pcg_iterations, st.rng_state, st.n_markers) == (rec["substeps"], rec["iterations"], rec["rng_state"], len(rec["markers"])), what
        for fld, name in MASKS:
            assert_bits(sim.get(fld), rec[name], "%s %s" % (what, name))
        assert_bits(sim.get(ea.F_MARKERS), rec["markers"], what + " markers")
        assert_bits(sim.get(ea.F_U), rec["u"], what + " u")
        assert_bits(sim.get(ea.F_V), rec["v"], what + " v")
        assert totals(sim) == rec["stats"] and sim.time == rec["time"], what
        if rainbow:
            for fld, q in zip((ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B), rec["dye"]):
                assert_bits(sim.get(fld), q, "%s dye %d" % (what, fld))
        if heat:
            assert_bits(sim.temperature, rec["T"], what + " T")
    sim.close()
    last = want[-1]["stats"]
    assert last["removed"] > 0 and last["cells_thinned"] > 0, last      # the pass had work to do
    return last


@pytest.mark.parametrize("scene", ["dam_break", "waterfall"])
@pytest.mark.parametrize("size", GRIDS)
def test_free_run(am, size, scene):
    last = free_run(am, size, scene)
    print(size, scene, last)


# Every variant below runs in the lean forms (no option) and with each lean form switched off, alone and all three together: the dye's and the temperature's
# extension, the sources and extrapolate read the tile map and the counts right after the pass has rewritten them.  All hold the device to the SAME restated
# run (computed once per variant), so the forms agree with each other bit for bit.
FORMS = [()] + [(o,) for o in LEAN_OFF] + [LEAN_OFF]
FORM_IDS = ["lean", "no_tile_map", "markers_two_pass", "markers_rowmajor", "all_three_off"]


@pytest.mark.parametrize("options", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rk2,mc", [(1, 0), (0, 1), (1, 1)])
def test_free_run_under_rk2_and_maccormack(am, rk2, mc, options):
    free_run(am, (101, 45), "waterfall", rk2=rk2, mc=mc, options=options)


@pytest.mark.parametrize("options", FORMS, ids=FORM_IDS)
def test_free_run_with_the_dye(am, options):
    free_run(am, (96, 64), "waterfall", rainbow=True, options=options)


@pytest.mark.parametrize("options", FORMS, ids=FORM_IDS)
def test_free_run_with_a_forcing(am, options):
    free_run(am, (101, 45), "dam_break", forced=True, options=options)


@pytest.mark.parametrize("options", FORMS, ids=FORM_IDS)
def test_free_run_with_heat_on(am, options):
    free_run(am, (96, 64), "dam_break", heat=True, options=options)


@pytest.mark.parametrize("options", FORMS[1:], ids=FORM_IDS[1:])
@pytest.mark.parametrize("scene,size", [("waterfall", (130, 70)), ("dam_break", (96, 64)), ("waterfall", (101, 45))])
def test_the_full_forms_give_the_same_bits(am, scene, size, options):
    """the plain RK1 run of test_free_run (which holds the lean forms to the same restatement) with the lean forms switched off"""
    free_run(am, size, scene, options=options)


# ----------------------------------------------------------------------------- a filled hole that is the only water of its tile
CORNER = (64, 64)      # the first cell of tile (1, 1) of the tile map on 130 x 70


@functools.lru_cache(maxsize=None)
def corner_state():
    """130 x 70: tile (1, 1) - columns 64 .., rows 64 .. - holds no marker at all.  Cell (64, 64) was water a refresh ago and is empty; its five neighbours in the
    tiles (0, 0), (1, 0) and (0, 1) are wet, the three inside its own tile - (65, 64), (64, 65), (65, 65) - are solid: a hole, and once filled the only water of
    its tile, whose flag the refresh has just cleared."""
    X, Y = 130, 70
    st = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in eref.synthetic_state(X, Y, 91, (5 * X * Y) // 4).items()}
    for n in ("solid", "sink", "source"):
        st[n][62:67, 62:67] = 0
    st["source"][64:, 64:] = 0      # (a source cell would put water - and its own flag - into the tile in the source stage)
    for cx, cy in ((65, 64), (64, 65), (65, 65)):
        st["solid"][cy, cx] = 1
    m = st["markers"]
    fx, fy = np.floor(m[:, 0]), np.floor(m[:, 1])
    m = m[~((fx >= 64) & (fy >= 64)) & ~((fx >= 62) & (fx <= 66) & (fy >= 62) & (fy <= 66))]
    wet = [(63, 63), (64, 63), (65, 63), (63, 64), (63, 65)]
    m = np.concatenate([m, np.array([(x + 0.5, y + 0.5) for x, y in wet], F32)])
    st["markers"] = np.ascontiguousarray(m, F32)
    count = eref.bins(st["markers"], X, Y)
    count[CORNER[1], CORNER[0]] = 1
    st["count"], st["prev_count"] = count, count.copy()
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


@pytest.mark.parametrize("mode", ["parity", "tile"])
def test_a_filled_hole_that_is_the_only_water_of_its_tile(am, mode):
    """one pass against the restatement, then the rest of the substep and two more frames in the lean forms against EULER_OPT_NO_TILE_MAP: the pass must flag the
    tile it fills, or the one-grid readers of the map (the assembly, the velocity update) and the next refresh pass the cell by"""
    st, r = corner_state(), rref.reseed(0, True)
    cx, cy = CORNER
    kw = {} if mode == "parity" else dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=200)      # (tile: the one-grid readers of the map)
    a, o, stats = both_passes(st, r, **kw)
    compare(a, o, "corner", stats)
    count = np.array(o.count)
    assert count[cy, cx] == 1 and count[64:, 64:].sum() == 1 and stats["added"] == 1
    assert (np.floor(np.array(o.markers)) == np.array([cx, cy], F32)).all(axis=1).sum() == 1
    b = load_state(ea.Simulation(st["X"], st["Y"], **kw), st)
    b.set_option(ea.OPT_NO_TILE_MAP, 1)
    b.set_reseed(record(r))
    b.stage(ea.STAGE_REFRESH_COUNTS)
    dt = float(F32(0.01))
    for s in (a, b):
        for stage in range(ea.STAGE_SOURCES, ea.STAGE_PROJECT + 1):
            s.stage(stage, dt)
    wet = a.get(ea.F_COUNT) != 0
    assert wet[cy, cx] and wet[64:, 64:].sum() == 1      # still the only water of its tile
    for fld in STATE_FIELDS:
        x, y = a.get(fld), b.get(fld)
        if fld == ea.F_PRESSURE:
            x, y = np.where(wet, x, 0.0), np.where(wet, y, 0.0)
        assert_bits(x, y, "behind the substep, field %d" % fld)
    a.stage(ea.STAGE_REFRESH_COUNTS); b.stage(ea.STAGE_REFRESH_COUNTS)      # the next refresh rotates the filled cell's count into prev_count
    assert a.get(ea.F_PREV_COUNT)[cy, cx] == 1
    for k in range(2):
        a.step(); b.step()
        for fld in (ea.F_U, ea.F_V, ea.F_COUNT, ea.F_PREV_COUNT, ea.F_MARKERS):
            assert_bits(a.get(fld), b.get(fld), "frame %d field %d" % (k, fld))
    assert a.stats().rng_state == b.stats().rng_state and totals(a) == totals(b)
    a.close(); b.close(); o.close()


# ----------------------------------------------------------------------------- the properties
def test_set_and_cleared_leaves_no_trace():
    def make():
        s = ea.Simulation(130, 70).load_text(scenarios.waterfall(), upscale=True)
        s.profile_enable(ea.profile_class_names())
        return s

    a, b, c = make(), make(), make()
    b.set_reseed(thin_above=5, fill_holes=True)
    c.set_reseed(thin_above=5, fill_holes=True)
    b.clear_reseed()
    assert int(b.reseed()[0]["thin_above"]) == 0 and int(c.reseed()[0]["thin_above"]) == 5
    for s in (a, b, c):
        s.profile_reset()
    for _ in range(6):
        a.step(); b.step(); c.step()
    la, lb, lc = launches(a), launches(b), launches(c)
    assert la == lb, {k: (la.get(k), lb.get(k)) for k in set(la) | set(lb) if la.get(k) != lb.get(k)}
    assert sum(lc.values()) > sum(la.values()) and totals(c)["removed"] > 0      # (and a handle with it on does run more)
    for fld in STATE_FIELDS:
        assert_bits(b.get(fld), a.get(fld), "field %d" % fld)
    assert a.stats().rng_state == b.stats().rng_state and totals(b) == rref.new_stats()
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("size", GRIDS)
def test_nothing_crowded_and_no_hole_changes_nothing(size):
    """the dam break as loaded and three frames on: four markers a cell and no hole yet with a bound of 200 - no marker, no count, no RNG bit moves, the totals stay 0"""
    a = ea.Simulation(*size).load_text(scenarios.dam_break(), upscale=True)
    b = ea.Simulation(*size).load_text(scenarios.dam_break(), upscale=True)
    for k in range(4):
        b.set_reseed(thin_above=200, fill_holes=k == 0)      # (the water as loaded has no hole; once it moves, single cells do open)
        a.stage(ea.STAGE_REFRESH_COUNTS); b.stage(ea.STAGE_REFRESH_COUNTS)
        for fld in STATE_FIELDS:
            assert_bits(b.get(fld), a.get(fld), "frame %d field %d" % (k, fld))
        assert a.stats().rng_state == b.stats().rng_state and a.stats().n_markers == b.stats().n_markers and totals(b) == rref.new_stats()
        a.step(); b.step()
    a.close(); b.close()


@pytest.mark.parametrize("size", GRIDS)
def test_the_diagnostics_right_after_a_pass_agree_with_the_counts(size):
    sim, o, stats = both_passes(planted_state(*size), rref.reseed(16, True))
    d = sim.diagnostics()
    count, solid = sim.get(ea.F_COUNT)[1:-1, 1:-1], sim.get(ea.F_SOLID)[1:-1, 1:-1]
    fluid = (count > 0) & (solid == 0)
    assert (d["fluid"], d["markers"], d["crowded"], d["count_max"]) == (int(fluid.sum()), int(count[fluid].sum()), int((count[fluid] >= 8).sum()), int(count[fluid].max()))
    assert d["count_max"] <= 16
    sim.close(); o.close()


@pytest.mark.parametrize("thin", [16, 5])
@pytest.mark.parametrize("precond", [ea.PRECOND_IC0_TILE, ea.PRECOND_IC0_TILE_MG])
def test_the_bound_holds_in_the_other_solver_modes(precond, thin):
    """a thinned cell keeps one marker per sub-cell, at most 16: with thin_above = 16 the count never exceeds thin_above at a frame's end (the source stage behind
    the pass only adds to cells below 4); a lower bound thins earlier - it has work in every frame of this run - and still leaves at most 16"""
    sim = ea.Simulation(130, 70, dot_mode=ea.DOT_TREE, precond=precond, max_iterations=200).load_text(scenarios.waterfall(), upscale=True)
    sim.set_reseed(thin_above=thin, fill_holes=True)
    for k in range(30):
        sim.step()
        assert sim.diagnostics()["count_max"] <= 16 and int(sim.get(ea.F_COUNT).max()) <= 16, k
    t = totals(sim)
    assert (t["removed"] > 0 or thin == 16) and t["added"] > 0 and sim.stats().n_markers > 0
    sim.close()


# ----------------------------------------------------------------------------- the interface
def test_refusals_in_order_and_the_lifetime_of_the_settings(tmp_path):
    X, Y = 96, 64
    sim = ea.Simulation(X, Y)
    L = sim.L
    good = record(rref.reseed(16, True, 100, 50)).reshape(1)

    def call(s, r=good):
        return L.euler_set_reseed(s.h if s else None, r.ctypes.data if r is not None else None)

    def bad(**kw):
        r = good.copy()
        for k, v in kw.items():
            r[k][0] = v
        return r

    assert call(None) == EULER_EINVAL                                                                   # 1: a null handle
    assert call(sim, bad(reserved=(0, 0, 1, 0), thin_above=3)) == EULER_ESTATE                          # 3: nothing loaded, in front of the record
    sim.load_text(scenarios.dam_break(), upscale=True)
    before = sim.hbm_bytes()
    state = [sim.get(fld) for fld in STATE_FIELDS]
    order = [(bad(reserved=(0, 0, 0, 7), thin_above=3, fill_holes=2, max_cells=-1, max_fill=-1), b"reserved"),      # 4, in this order
             (bad(thin_above=3, fill_holes=2, max_cells=-1, max_fill=-1), b"thin_above"), (bad(thin_above=255), b"thin_above"), (bad(thin_above=-16), b"thin_above"),
             (bad(fill_holes=2, max_cells=-1, max_fill=-1), b"fill_holes"), (bad(fill_holes=-1), b"fill_holes"),
             (bad(max_cells=-1, max_fill=-1), b"max_cells"), (bad(max_cells=(1 << 20) + 1), b"max_cells"), (bad(max_fill=-1), b"max_fill"), (bad(max_fill=(1 << 20) + 1), b"max_fill")]
    for r, word in order:
        assert call(sim, r) == EULER_EINVAL and word in L.euler_last_error(), (word, L.euler_last_error())
    # a refused call changes and allocates nothing
    assert sim.hbm_bytes() == before and sim.reseed()[0].tobytes() == bytes(32)
    for fld, a in zip(STATE_FIELDS, state):
        assert_bits(sim.get(fld), a, "field %d" % fld)
    # set: the record comes back as given, the pass's buffers are allocated once; NULL and all-zero switch it off
    assert call(sim) == 0 and sim.hbm_bytes() > before
    held = sim.hbm_bytes()
    assert sim.reseed()[0].tobytes() == good.tobytes()
    assert call(sim, bad(thin_above=1)) == EULER_EINVAL and sim.reseed()[0].tobytes() == good.tobytes()      # a refusal leaves the record as set
    assert call(sim, None) == 0 and sim.reseed()[0].tobytes() == bytes(32) and sim.hbm_bytes() == held
    assert call(sim, bad(thin_above=254, max_cells=1 << 20, max_fill=0)) == 0 and call(sim, bad(thin_above=0, fill_holes=0)) == 0
    assert int(sim.reseed()[0]["max_cells"]) == 100      # the limits as given, the pass off
    assert L.euler_get_reseed(None, None, None) == EULER_EINVAL and L.euler_get_reseed(sim.h, None, None) == 0
    # the settings survive a scenario load and euler_load_state, the totals a load; a new set zeroes them
    sim.set_reseed(thin_above=5, fill_holes=True)
    for _ in range(6):
        sim.step()
    t = totals(sim)
    assert t["removed"] > 0
    snap = str(tmp_path / "state.snap")
    sim.save_state(snap)
    sim.load_state(snap)
    assert int(sim.reseed()[0]["thin_above"]) == 5 and totals(sim) == t
    sim.load_text(scenarios.dam_break(), upscale=True)
    assert int(sim.reseed()[0]["thin_above"]) == 5 and int(sim.reseed()[0]["fill_holes"]) == 1 and totals(sim) == t
    n0 = sim.stats().n_markers
    for _ in range(6):
        sim.step()
    assert totals(sim)["removed"] == 2 * t["removed"] and sim.stats().n_markers == n0 - t["removed"] + t["added"]      # the same run again, counted on
    sim.set_reseed(thin_above=5, fill_holes=True)
    assert totals(sim) == rref.new_stats()
    with pytest.raises(ea.EulerError) as e:
        sim.set_reseed(thin_above=300)
    assert e.value.code == EULER_EINVAL and "thin_above" in str(e.value)
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    assert call(slab, bad(reserved=(1, 0, 0, 0))) == EULER_ESTATE and b"slab" in L.euler_last_error()      # 2: in front of "nothing loaded" and of the record
    slab.close()


def test_cli_reseed(tmp_path):
    X, Y = 100, 40
    text = scenarios.waterfall()
    scn = tmp_path / "waterfall.txt"
    scn.write_text(text)
    base = [EXE, "--dump", "--window", "98x38", "--size", "%dx%d" % (X, Y)]

    def run(*flags, frames=25):
        r = subprocess.run(base + ["--frames", str(frames)] + list(flags) + [str(scn)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout, r.stderr.decode()

    def driven(frames, **kw):
        sim = ea.Simulation(X, Y).load_text(text)
        if kw:
            sim.set_reseed(**kw)
        out = [sim.draw(98, 38)]
        for _ in range(frames):
            sim.step()
            out.append(sim.draw(98, 38))
        t = totals(sim) if kw else None
        sim.close()
        return out, t

    for spec, kw in (("16:fill", dict(thin_above=16, fill_holes=True)), ("5:fill", dict(thin_above=5, fill_holes=True)), ("5", dict(thin_above=5)), ("0:fill", dict(fill_holes=True))):
        out, err = run("--reseed", spec)
        want, t = driven(25, **kw)
        assert dumped_frames(out) == want, spec
        line = [ln for ln in err.splitlines() if ln.startswith("reseed ")]
        assert line == ["reseed removed %d added %d cells_thinned %d deferred %d" % (t["removed"], t["added"], t["cells_thinned"], t["deferred"])], (spec, err)
    assert t["added"] > 0
    # without the flag: the frames of a plain run and no such line
    out, err = run(frames=5)
    assert dumped_frames(out) == driven(5)[0] and "reseed" not in err
    # usage errors and refused values: status 1
    for flags, word in ((["--reseed", "fill"], b"usage"), (["--reseed", "16:"], b"usage"), (["--reseed", "16:fil"], b"usage"), (["--reseed", "16x"], b"usage"),
                        (["--reseed", "3"], b"thin_above"), (["--reseed", "255:fill"], b"thin_above")):
        r = subprocess.run(base + ["--frames", "2"] + flags + [str(scn)], capture_output=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (flags, r.stderr)
