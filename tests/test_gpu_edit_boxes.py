"""euler_edit_box (docs/editing.md) on boxes the scenes of test_gpu_edit.py never place, bit for bit against tests/edit_ref.py: structured families of boxes and a
random chain on synthetic random states (96 x 64, 101 x 45, 260 x 200, 203 x 131: boxes of several cell-pass workgroups, columns of the eligibility mask taller than
64, every alignment of the dword path's edges, markers exactly on a box's edges), the three-launch ordered select, compactions of millions of markers and RNG jumps
of millions of draws on 2048 x 1100, and one continuation over a tile map of 5 x 4 tiles, device edit against a load of the host-edited snapshot.
test_edit_host.py holds the states and the boxes to what these tests need of them."""
import time

import numpy as np
import pytest

import edit_ref as er
import euler_amd as ea
from euler_amd import scenarios
from observer_util import EULER_EINVAL
from test_gpu_edit import GRID_FIELDS, RUN_FIELDS, assert_state, dam_break, load_state, read_state, same_run
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

ALL = tuple(GRID_FIELDS)


def edit(sim, st, op, box, what):
    """the edit on the handle and on the restated state `st`, compared on every grid, the markers in order, n, the RNG and the latch -> the restated state after it"""
    try:
        want = er.edit_state(st, er.OPS[op], box)
    except er.Refused:
        with pytest.raises(ea.EulerError) as e:
            sim.edit_box(er.OPS[op], box)
        assert e.value.code == EULER_EINVAL, what
        want = st
    else:
        sim.edit_box(er.OPS[op], box)
    assert_state(sim, want, what, fields=ALL)
    return want


# ----------------------------------------------------------------------------- 1. structured boxes, all ops; a random chain
@pytest.mark.parametrize("grid", list(er.BOX_GRIDS))
def test_box_families_and_a_random_chain_equal_the_restatement(grid):
    """one handle per grid, the synthetic state loaded afresh before every case of er.box_families; then without reloading: DRAIN of everything (D = n), a DRAIN
    with no marker left, FILL of everything; 12 seeded random (op, box) pairs; five ops from the synthetic state of n = 0 - compared after every edit"""
    X, Y = grid
    t0 = time.perf_counter()
    plain = er.synthetic_state(X, Y, *er.BOX_GRIDS[grid])
    sim = load_state(ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL), plain)
    hbm = sim.hbm_bytes()
    edits = 0
    for family, cases in er.box_families(X, Y).items():
        for op, box in cases:
            st = er.family_state(X, Y, family, box)
            load_state(sim, st)
            after = edit(sim, st, op, box, "%s %s: %s %s" % (grid, family, op, box))
            if family == "edge markers" and op in ("solid", "sink", "drain"):      # the four of the eight that lie in the box are gone, the other four are not
                e, inside = er.edge_markers(box)
                left = {tuple(p) for p in after["markers"].tolist()}
                assert [tuple(p) in left for p in e.tolist()] == list(~inside), (grid, op, box)
            edits += 1
    whole = (1, 1, X - 2, Y - 2)
    st = plain
    load_state(sim, st)
    for op, box in (("drain", whole), ("drain", (2, 2, 9, 9)), ("fill", whole)):
        st = edit(sim, st, op, box, "%s everything: %s %s" % (grid, op, box))
        assert len(st["markers"]) == (0 if op == "drain" else 4 * int(((plain["solid"] == 0) & (plain["sink"] == 0))[1:-1, 1:-1].sum()))
    seed = 1000 + list(er.BOX_GRIDS).index(grid)
    print("%s: random chain, seed %d" % (grid, seed))
    st = plain
    load_state(sim, st)
    for k, (op, box) in enumerate(er.random_chain(X, Y, seed)):
        n = len(st["markers"])
        st = edit(sim, st, op, box, "%s chain seed %d, edit %d: %s %s" % (grid, seed, k, op, box))
        print("  %d %-6s %-22s %6d -> %6d markers" % (k, op, box, n, len(st["markers"])))
    # the synthetic state without a marker, as loaded: the deleting ops find nothing to select, the seeding ops append at n = 0
    st = er.synthetic_state(X, Y, er.BOX_GRIDS[grid][0], 0)
    load_state(sim, st)
    for op, box in (("drain", (2, 2, X // 2, Y // 2)), ("solid", (3, 3, 7, 5)), ("fill", (1, 1, X // 2 + 3, Y - 2)), ("sink", whole), ("source", (5, 2, X - 3, 9))):
        st = edit(sim, st, op, box, "%s no markers: %s %s" % (grid, op, box))
    assert len(st["markers"]) == 4 * (X - 7) * 8
    load_state(sim, plain)
    assert sim.hbm_bytes() == hbm
    sim.close()
    print("%s: %d structured edits + 3 + 12 + 5 in %.2f s" % (grid, edits, time.perf_counter() - t0))


# ----------------------------------------------------------------------------- 2. the long paths
LONG = (2048, 1100)      # the interior exceeds 2^21 cells
LONG_MARKERS = 2788920   # the upscaled dam break as loaded: 1.33 x 2^21 (parse_scenario + seed_markers; the half tank has 4.5 M, and every pass takes longer)


def test_long_select_large_compaction_and_far_jumps():
    """2048 x 1100, the upscaled dam break as loaded - 2 788 920 markers, 1.33 x 2^21: eu_ordered_select's three-launch path on the delete mask and on the
    eligibility mask, k_compact_markers with D of more than a million and with D = n, eu_rng_jump over 16 M draws, columns of the eligibility mask 1098 bits tall.
    The whole state against the restatement after every edit; then one step from the last state: count is the bins of the markers it left, and the run is finite."""
    X, Y = LONG
    t0 = time.perf_counter()
    solid, source, sink, fluid = ea.parse_scenario(scenarios.dam_break(), X, Y, upscale=True)
    m0, rng0 = ea.seed_markers(fluid)
    assert len(m0) == LONG_MARKERS and LONG_MARKERS > 1.1 * (1 << 21)
    sim = ea.Simulation(X, Y).load_text(scenarios.dam_break(), upscale=True)
    hbm = sim.hbm_bytes()
    st = read_state(sim)
    assert_bits(st["markers"], m0, "the loaded markers")
    assert st["rng_state"] == rng0 and np.array_equal(st["solid"], solid) and np.array_equal(st["sink"], sink)
    sim.profile_enable(["select", "marker_compact"])

    def run(op, box, what):
        sim.profile_reset()
        n = len(st["markers"])
        t = time.perf_counter()
        after = edit(sim, st, op, box, what)
        p = sim.profile()
        k = {c: int(p.get(c, (0.0, 0))[1]) for c in ("select", "marker_compact")}
        print("%-34s %-22s %8d -> %8d markers, launches %s, %.2f s" % (what, box, n, len(after["markers"]), k, time.perf_counter() - t))
        return after, k

    cells = lambda b: (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
    # (three launches: the mask has more than SEL1_MAX_WORDS = 1 << 15 words, k_markers.hip)
    n = len(st["markers"])
    st, k = run("drain", (47, 1, 600, 1098), "DRAIN half the water")
    assert (n + 63) // 64 > 1 << 15 and k == {"select": 3, "marker_compact": 1}, k
    assert 1 << 20 < n - len(st["markers"]) < n and abs(2 * len(st["markers"]) - n) < n // 10      # (D = 1 407 160: about half)
    st, k = run("drain", (1, 1, X - 2, Y - 2), "DRAIN everything")
    assert len(st["markers"]) == 0 and k["marker_compact"] == 1
    box = (3, 1, 2045, 1098)
    st, k = run("fill", box, "FILL")
    assert cells(box) > 1 << 21 and (cells(box) + 63) // 64 > 1 << 15 and k == {"select": 3, "marker_compact": 0}, k
    E = len(st["markers"]) // 4
    assert E > 1000000 and 8 * E > 8000000      # (the last cell's draws start 8 (E - 1) draws down the stream)
    n = len(st["markers"])
    st, k = run("solid", (1, 500, X - 2, 560), "SOLID across the new water")
    assert n - len(st["markers"]) > 400000 and k == {"select": 3, "marker_compact": 1}, k
    box = (1, 1, X - 2, Y - 2)
    n = len(st["markers"])
    st, k = run("source", box, "SOURCE over the interior")
    assert cells(box) >= 1 << 21 and len(st["markers"]) - n > 4 * 2000 * 61 and k == {"select": 3, "marker_compact": 0}, k
    # a small edit on the same handle: the short path, one launch (the delete mask is as long as the marker array: DRAIN takes three whatever its box)
    st, k = run("drain", (10, 10, 12, 12), "a small DRAIN")
    assert k == {"select": 3, "marker_compact": 1}, k
    st, k = run("fill", (10, 10, 12, 12), "a small FILL")
    assert k == {"select": 1, "marker_compact": 0}, k
    assert sim.hbm_bytes() == hbm
    sim.profile_enable([])
    t = time.perf_counter()
    sim.step()
    s = read_state(sim)
    print("one step: %d substeps, %d PCG iterations, %d markers, %.2f s" % (sim.stats().last_substeps, sim.stats().last_pcg_iterations, len(s["markers"]), time.perf_counter() - t))
    assert np.isfinite(s["u"]).all() and np.isfinite(s["v"]).all() and np.isfinite(s["markers"]).all()
    # count is what the last refresh binned plus what the sources behind it appended (main.c:287-289): every marker once, in the cell it lies in, none in a sink
    # or solid cell.  (Exact for this seeded run.  A source marker at x + randf() that rounds up to x + 1 in float would count in the cell that drew it until the
    # next refresh - 6e-5 per draw at x = 2000, and the step draws 578 times: should a change to the scene above ever make one, that cell and its neighbour show here.)
    assert int(s["count"].astype(np.int64).sum()) == len(s["markers"]) and s["count"].max() < 255
    b = er.bins(s["markers"], X, Y)
    b[(s["solid"] != 0) | (s["sink"] != 0)] = 0
    bad = np.argwhere(s["count"] != b)
    print("count != bins in %d cells" % len(bad))
    assert len(bad) == 0, bad[:8]
    sim.close()
    print("the long paths: %.2f s" % (time.perf_counter() - t0))


# ----------------------------------------------------------------------------- 3. one multi-tile continuation, GPU against GPU
MULTI = (260, 200)      # a tile map of 5 x 4 tiles
MULTI_EDITS = (("solid", (60, 60, 70, 70)),        # across the corner of four tiles, in the falling block
               ("fill", (200, 50, 240, 80)),       # two tiles without water
               ("drain", (100, 100, 140, 150)),    # a hole in the block across x = 128 and y = 128 (not around the wall: the water above it falls onto it, a solve in every substep)
               ("source", (120, 180, 135, 184)))   # under the ceiling, across x = 128
MULTI_MODES = {
    "parity": dict(dot_mode=ea.DOT_SEQUENTIAL),
    "tile_resident_off": dict(precond=ea.PRECOND_IC0_TILE, dot_mode=ea.DOT_TREE, resident=ea.RESIDENT_OFF),
}


@pytest.mark.parametrize("mode", list(MULTI_MODES))
def test_multi_tile_device_edit_equals_load_of_host_edited_snapshot(mode, tmp_path):
    """test_gpu_edit.py's device edit against a load of the host-edited snapshot, at 260 x 200 after 4 frames of the upscaled dam break: 6 frames, the run's fields and
    counters bit for bit; the unedited control of the mode first"""
    kw = MULTI_MODES[mode]
    make = lambda: dam_break(MULTI, **kw)
    path = str(tmp_path / "state.snap")
    a, b = make(), make()
    b.save_state(path)
    b.load_state(path)
    same_run(a, b, RUN_FIELDS, 6, mode + " control")
    a.close(); b.close()
    a, b = make(), make()
    count = a.get(ea.F_COUNT)
    assert count[60:71, 60:71].all() and count[100:151, 100:141].all() and not count[0:128, 192:256].any()      # water where SOLID and DRAIN go, none in FILL's two tiles
    for name, box in MULTI_EDITS:
        a.edit_box(er.OPS[name], box)
    b.save_state(path)
    snap = ea.read_snapshot(path)
    n0 = len(snap["markers"])
    for name, box in MULTI_EDITS:
        snap = er.edit_state(snap, er.OPS[name], box)
    ea.write_snapshot(path, snap)
    b.load_state(path)
    for fld in RUN_FIELDS:
        assert_bits(a.get(fld), b.get(fld), "%s edited, field %d" % (mode, fld))
    s = same_run(a, b, RUN_FIELDS, 6, mode)
    print("%s: %d -> %d markers by the edits, %d at the end, %d PCG iterations in all" % (mode, n0, len(snap["markers"]), s.n_markers, s.total_pcg_iterations))
    assert s.total_pcg_iterations > 1000      # (the oracle from the restated state: 13 substeps in the 6 frames, each at the cap of 100)
    a.close(); b.close()
