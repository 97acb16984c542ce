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
