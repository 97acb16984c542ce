"""The numpy restatement of euler_edit_box (tests/edit_ref.py) held to the reference, and the scenes of the GPU edit tests held to what those tests need of
them - with the oracle alone, no GPU."""
import numpy as np
import pytest

import edit_ref as er
import euler_amd as ea
from euler_amd import scenarios
from golden_util import X, Y, load, scenario_text
from test_gpu_parity import assert_bits

CASES = [(g, w) for g in er.GRIDS for w in list(er.BOXES_96x64) + ["sequence"]]


def seeded_home_bins(before, after):
    """The bins of `after`'s markers, where the markers seeded behind those of `before` (cells in column-major order over the cells that gained a count of 4, four each)
    count in the cell that seeded them.  A seeded marker outside its cell lies exactly on the cell's far edge (j + 0.5 + a jitter just below 0.5 rounds to j + 1 in
    float, or a draw of exactly 1.0): the edit does not special-case it, and the next refresh counts it where it lies.  -> (bins, the cells such markers left and lie in)"""
    Yg, Xg = after["count"].shape
    m = np.asarray(after["markers"])
    n_old = len(m) - 4 * int(((after["count"] == 4) & (before["count"] == 0)).sum())
    c = er.bins(m[:n_old], Xg, Yg).astype(np.int64)
    ys, xs = np.nonzero(((after["count"] == 4) & (before["count"] == 0)).T)[::-1]      # x outer, y inner
    away = set()
    for k, (cx, cy) in enumerate(zip(xs, ys)):
        for q in range(4):
            mx, my = m[n_old + 4 * k + q]
            c[cy, cx] += 1
            if (np.floor(mx), np.floor(my)) != (cx, cy):
                assert (mx == cx + 1 and cx <= mx) or (my == cy + 1 and cy <= my), (cx, cy, mx, my)
                assert cx <= mx <= cx + 1 and cy <= my <= cy + 1
                away |= {(int(cx), int(cy)), (int(np.floor(mx)), int(np.floor(my)))}
    return (c % 256).astype(np.uint8), away


@pytest.mark.parametrize("grid,what", CASES)
def test_count_grid_is_the_bins_of_the_markers(grid, what):
    """after every op (and after the six in sequence) the restated count grid is what a refresh would count - a seeded marker on its cell's far edge counted at home"""
    st = er.base_state(*grid)
    assert np.array_equal(st["count"], er.bins(st["markers"], *grid))
    stray = set()      # cells whose count and bins differ by a seeded marker on a far edge, from the op that seeded it on
    for name in er.SEQUENCE if what == "sequence" else (what,):
        nxt = er.edit_state(st, er.OPS[name], er.scaled_box(name, *grid))
        if name in ("fill", "source"):
            got, away = seeded_home_bins(st, nxt)
            if not stray:
                assert np.array_equal(nxt["count"], got), (grid, what, name)
            stray |= away
        ys, xs = np.nonzero(nxt["count"] != er.bins(nxt["markers"], *grid))
        assert set(zip(xs.tolist(), ys.tolist())) <= stray, (grid, what, name)
        x0, y0, x1, y1 = er.scaled_box(name, *grid)
        for f in ("u", "v", "utmp", "vtmp", "prev_count", "precon"):      # not touched
            assert_bits(nxt[f], st[f], f)
        outside = np.ones(st["count"].shape, bool)
        outside[y0:y1 + 1, x0:x1 + 1] = False
        for f in ("solid", "source", "sink", "count"):
            assert np.array_equal(nxt[f][outside], st[f][outside]), (name, f)
        st = nxt
    assert len(stray) <= 2      # (the 96 x 64 FILL box has one such marker: cell (77, 42)'s, at y = 43.0)


def test_anchor_drain_and_fill_reproduce_the_loaded_marker_array():
    """On the dam break as loaded: DRAIN the whole interior, the RNG back at the initial seed, FILL the block's rectangle - sim_init's marker array bit for bit, in order
    (the golden fixture's frame 0 is the compiled reference's)."""
    g = load("block_frames.npz")
    text = scenario_text(g)
    solid, source, sink, fluid = ea.parse_scenario(text, X, Y)
    loaded, rng_after = ea.seed_markers(fluid)
    o = er.parity_oracle(er.moving_state(X, Y, text, 0, upscale=False))
    assert_bits(np.array(o.markers), loaded, "the oracle's sim_init")
    st = er.moving_state(X, Y, text, 0, upscale=False)
    o.close()
    drained = er.edit_state(st, ea.EDIT_DRAIN, (1, 1, X - 2, Y - 2))
    assert len(drained["markers"]) == 0 and not drained["count"].any()
    drained["rng_state"] = 0x9bd185c449534b91      # EULER_RNG_SEED (include/euler.h)
    ys, xs = np.nonzero(fluid)
    box = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
    assert fluid[box[1]:box[3] + 1, box[0]:box[2] + 1].all()      # the block is a rectangle
    filled = er.edit_state(drained, ea.EDIT_FILL, box)
    assert_bits(filled["markers"], np.asarray(st["markers"]), "markers")
    assert filled["rng_state"] == rng_after == st["rng_state"]
    assert np.array_equal(filled["count"], st["count"])
    if "markers0" in g.files:
        assert_bits(filled["markers"], g["markers0"], "the reference's frame 0")


def test_delete_is_the_sequential_loop_and_keeps_the_multiset():
    st = er.base_state(96, 64)
    box = er.scaled_box("drain", 96, 64)
    m = np.asarray(st["markers"])
    keep = np.array([not er.in_box(x, y, box) for x, y in m])
    out = er.delete_in_box(m, box)
    from oracle_lib import sort_markers
    assert_bits(sort_markers(out), sort_markers(m[keep]), "survivors")
    n1 = len(out)
    assert_bits(out[:n1][keep[:n1]], m[:n1][keep[:n1]], "survivors in front stay in place")
    assert not np.array_equal(out, m[keep])      # (the order is NOT that of a stable compaction: holes are filled from the back)


def test_capacity_refusal():
    st = er.base_state(96, 64)
    full = dict(st)
    full["markers"] = np.tile(np.array([[50.5, 50.5]], np.float32), (4 * 96 * 64 - 10, 1))
    with pytest.raises(er.Refused):
        er.edit_state(full, ea.EDIT_FILL, (70, 40, 85, 50))
    assert len(er.edit_state(full, ea.EDIT_FILL, (70, 40, 71, 40))["markers"]) == 4 * 96 * 64 - 2      # 8 more fit: n + 4 E = max - 2


@pytest.mark.parametrize("grid", er.GRIDS)
def test_scenes_show_what_the_gpu_tests_need(grid):
    """Every op changes the marker count or the later trajectory, the run stays finite, and the frames after the edit have PCG iterations; the FILL box lies in a tile
    without water (96 x 64, 101 x 45).  96 x 64: the marker counts and iteration totals recorded when the scenes were chosen."""
    base = er.base_state(*grid)
    plain = er.continued(grid[0], grid[1], None)
    assert sum(r["iterations"] for r in plain) > 1000
    x0, y0, x1, y1 = er.scaled_box("fill", *grid)
    tx, ty = x0 // 64, y0 // 64
    dry = not base["count"][64 * ty:64 * ty + 64, 64 * tx:64 * tx + 64].any()
    assert (x1 // 64, y1 // 64) == (tx, ty) and base["count"].any()
    assert dry == (grid != (130, 70))      # (130 x 70: the block reaches into the tile right of x = 64 - FILL next to water, the other case)
    for what in list(er.BOXES_96x64) + ["sequence"]:
        st = er.edited_state(grid[0], grid[1], what)
        run = er.continued(grid[0], grid[1], what)
        assert all(r["finite"] for r in run), what
        assert sum(r["iterations"] for r in run) > 1000, what
        changed = len(st["markers"]) != len(base["markers"]) or any(not np.array_equal(a["u"], b["u"]) for a, b in zip(run, plain))
        assert changed, what
        if what in ("solid", "drain"):
            assert len(st["markers"]) < len(base["markers"])
        if what in ("fill", "source"):
            assert len(st["markers"]) > len(base["markers"])
    if grid == (96, 64):
        n = {w: len(er.edited_state(96, 64, w)["markers"]) for w in [None] + list(er.BOXES_96x64)}
        assert n == {None: 7140, "solid": 6716, "fill": 7844, "drain": 6651, "clear": 7140, "sink": 7140, "source": 7188}
        it = {w: sum(r["iterations"] for r in er.continued(96, 64, w)) for w in (None, "fill", "drain", "clear", "sink")}
        assert it == {None: 5563, "fill": 5720, "drain": 4768, "clear": 5561, "sink": 5253}
    if grid == (101, 45):
        assert (len(base["markers"]), len(er.edited_state(101, 45, "solid")["markers"])) == (5088, 4784)
    if grid == (130, 70):
        assert (len(base["markers"]), len(er.edited_state(130, 70, "solid")["markers"])) == (10764, 10240)


def test_source_on_a_scene_without_sources_pours():
    """SOURCE keeps appending in the frames that follow (update_fluid_sources, main.c:276-298), CLEAR over the cells stops it"""
    run = er.continued(96, 64, "source")
    assert er.edited_state(96, 64, "source")["source"].sum() == 12 and not er.base_state(96, 64)["source"].any()
    assert len(run[5]["markers"]) > len(er.edited_state(96, 64, "source")["markers"])


# ----------------------------------------------------------------------------- the vectorised delete, the synthetic states and the boxes of test_gpu_edit_boxes.py
def _delete_cases():
    """(name, markers, box): random cases with n from 0 to about 300, and the named ones"""
    rng = np.random.default_rng(2024)
    cases = []
    for k in range(320):
        n = int(rng.integers(0, 301))
        x0, x1 = sorted(int(t) for t in rng.integers(1, 19, 2))
        y0, y1 = sorted(int(t) for t in rng.integers(1, 13, 2))
        m = np.stack([rng.uniform(0.5, 19.5, n), rng.uniform(0.5, 13.5, n)], axis=1).astype(np.float32)
        cases.append(("random %d" % k, m, (x0, y0, x1, y1)))
    box = (4, 3, 9, 7)
    inside = lambda n, s: np.stack([np.random.default_rng(s).uniform(4.0, 9.99, n), np.random.default_rng(s + 1).uniform(3.0, 7.99, n)], axis=1).astype(np.float32)
    outside = lambda n, s: np.stack([np.random.default_rng(s).uniform(10.0, 19.0, n), np.random.default_rng(s + 1).uniform(0.5, 13.0, n)], axis=1).astype(np.float32)
    cases.append(("no marker at all", np.zeros((0, 2), np.float32), box))
    cases.append(("nothing deleted", outside(101, 1), box))
    cases.append(("everything deleted", inside(77, 3), box))
    cases.append(("one marker, deleted", inside(1, 5), box))
    cases.append(("one marker, kept", outside(1, 7), box))
    cases.append(("the last marker deleted", np.concatenate([outside(40, 9), inside(1, 11)]), box))
    cases.append(("a run of deleted markers at the tail", np.concatenate([outside(30, 13), inside(3, 15), outside(8, 17), inside(12, 19)]), box))
    cases.append(("more deletions than survivors", np.concatenate([inside(20, 21), outside(7, 23), inside(30, 25), outside(4, 27), inside(2, 29)]), box))
    cases.append(("odd n", np.concatenate([outside(25, 31), inside(25, 33), outside(25, 35), inside(26, 37)]), box))
    e, _ = er.edge_markers(box)
    cases.append(("the eight edge markers alone", e, box))
    cases.append(("edge markers among others", np.concatenate([e[:3], outside(11, 39), e[3:6], inside(9, 41), e[6:]]), box))
    cases.append(("edge markers at the tail", np.concatenate([inside(5, 43), outside(5, 45), e]), box))
    return cases


def test_vectorised_delete_is_the_literal_loop():
    """er.delete_in_box_vectorised (what edit_state uses) against er.delete_in_box, the definition: bit for bit, in order"""
    cases = _delete_cases()
    assert len(cases) >= 300
    seen = set()
    for name, m, box in cases:
        want = er.delete_in_box(m, box)
        got = er.delete_in_box_vectorised(m, box)
        assert got.dtype == np.float32 and got.shape == want.shape, (name, got.shape, want.shape)
        assert_bits(got, want, name)
        n, d = len(m), len(m) - len(want)
        gone = np.array([er.in_box(x, y, box) for x, y in m], bool)
        seen |= {"none" if d == 0 else "all" if d == n else "some", "odd" if n % 2 else "even"}
        if n and gone[-1]:
            seen.add("last")
        if n > 2 and gone[-3:].all() and not gone.all():
            seen.add("tail run")
        if 2 * d > n and d < n:
            seen.add("more deleted than kept")
        if n == 0:
            seen.add("empty")
    assert seen >= {"none", "all", "some", "odd", "even", "last", "tail run", "more deleted than kept", "empty"}, seen
    # the edge markers are in or out of the box as floor() says: on x0 in, one ulp below out, on x1 + 1 out, one ulp below in
    box = (4, 3, 9, 7)
    e, inside = er.edge_markers(box)
    assert [bool(er.in_box(x, y, box)) for x, y in e] == list(inside)
    assert e.dtype == np.float32 and e[1, 0] < 4 and e[3, 0] < 10 and np.floor(e[1, 0]) == 3 and np.floor(e[3, 0]) == 9 and e[2, 0] == 10 and e[6, 1] == 8
    assert len(er.delete_in_box(e, box)) == 4


@pytest.mark.parametrize("grid", list(er.BOX_GRIDS))
def test_synthetic_states_and_box_families_show_what_the_gpu_test_needs(grid):
    """The synthetic state of every grid of test_gpu_edit_boxes.py is a consistent state, every family of boxes has, for FILL, an eligible and an ineligible cell and a
    marker in a box and one outside, and over the grids every op meets every family"""
    X, Y = grid
    seed, n = er.BOX_GRIDS[grid]
    st = er.synthetic_state(X, Y, seed, n)
    loaded = er.base_state(X, Y, 0)
    inner = (slice(1, -1), slice(1, -1))
    for f in ("solid", "sink", "source"):
        border = np.ones((Y, X), bool)
        border[inner] = False
        assert np.array_equal(st[f][border], loaded[f][border]), f
    frac = lambda a: a[inner].mean()
    assert 0.12 < frac(st["solid"]) < 0.18 and 0.02 < frac(st["sink"]) < 0.04 and 0.02 < frac(st["source"]) < 0.04
    assert not ((st["solid"].astype(int) + st["sink"] + st["source"])[inner] > 1).any()
    m = st["markers"]
    assert m.dtype == np.float32 and len(m) == n
    mx, my = np.floor(m[:, 0]).astype(int), np.floor(m[:, 1]).astype(int)
    assert mx.min() >= 1 and mx.max() <= X - 2 and my.min() >= 1 and my.max() <= Y - 2 and not st["solid"][my, mx].any()
    assert st["sink"][my, mx].any()      # (markers in sink cells: what a refresh would delete, the edit leaves)
    assert np.array_equal(st["count"], er.bins(m, X, Y)) and np.array_equal(st["prev_count"], st["count"]) and st["count"].max() < 255
    assert np.abs(st["u"]).max() <= 0.1 and st["u"][inner].any() and st["v"][inner].any() and not st["utmp"].any() and not st["vtmp"].any() and not st["precon"].any()
    assert st["rng_state"] > 0 and st["source_exhausted"] == 0
    fams = er.box_families(X, Y)
    for family, cases in fams.items():
        elig = inel = m_in = m_out = False
        for op, box in cases:
            s0 = er.family_state(X, Y, family, box)
            x0, y0, x1, y1 = box
            sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            e = (s0["solid"][sl] == 0) & (s0["sink"][sl] == 0) & (s0["count"][sl] == 0)
            fx, fy = np.floor(s0["markers"][:, 0]), np.floor(s0["markers"][:, 1])
            inb = (x0 <= fx) & (fx <= x1) & (y0 <= fy) & (fy <= y1)
            elig, inel, m_in, m_out = elig or e.any(), inel or not e.all(), m_in or inb.any(), m_out or not inb.all()
        assert elig and inel and m_in and m_out, (grid, family, elig, inel, m_in, m_out)
    assert len(er.synthetic_state(X, Y, seed, 0)["markers"]) == 0 and not er.synthetic_state(X, Y, seed, 0)["count"].any()


def test_every_op_meets_every_box_family():
    met, shapes = {}, {}
    for X, Y in er.BOX_GRIDS:
        for family, cases in er.box_families(X, Y).items():
            met.setdefault(family, set()).update(op for op, _ in cases)
            shapes.setdefault(family, []).extend((X, Y, b) for _, b in cases)
    assert set(met) == {"edge alignment", "single cell", "whole interior", "tall and narrow", "wide and flat", "across workgroups", "edge markers"}
    for family, ops in met.items():
        assert ops == set(er.OP_NAMES), (family, ops)
    # edge alignment: on both X % 4 == 0 grids all 16 (x0 & 3, x1 & 3) and one column at each residue, heights 1 .. 5
    for g in ((96, 64), (260, 200)):
        bs = [b for X, Y, b in shapes["edge alignment"] if (X, Y) == g]
        assert {(b[0] & 3, b[2] & 3) for b in bs if b[2] > b[0]} == {(a, c) for a in range(4) for c in range(4)}
        assert {b[0] & 3 for b in bs if b[2] == b[0]} == {0, 1, 2, 3} and {b[3] - b[1] + 1 for b in bs} == {1, 2, 3, 4, 5}
    for g in ((260, 200), (203, 131)):
        bs = [b for X, Y, b in shapes["tall and narrow"] if (X, Y) == g]
        assert {(b[2] - b[0] + 1, b[3] - b[1] + 1) for b in bs} >= {(w, h) for w in (1, 2, 3, 5) for h in (65, 67, 128, 129, g[1] - 2)}
    bs = [b for X, Y, b in shapes["across workgroups"]]
    assert {b[3] - b[1] + 1 for b in bs} == {66, 97, 131, 198} and min(b[2] - b[0] + 1 for b in bs) >= 70
    assert {((b[0] - (b[0] & ~3)), b[1] > 1) for X, Y, b in shapes["across workgroups"] if X % 4 == 0} >= {(1, True), (3, True)}      # (unaligned in x, off the floor in y)
    assert max(len([1 for X, Y, b in shapes[f] if (X, Y) == g]) for f in shapes for g in er.BOX_GRIDS) <= 24 and all(sum(len(c) for c in er.box_families(*g).values()) <= 90 for g in er.BOX_GRIDS)
