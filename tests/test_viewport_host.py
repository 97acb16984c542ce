"""The host half of the pan-and-zoom viewport (docs/viewport.md), no GPU: the numpy restatement (tests/viewport_ref.py) against its plain-loop
twin, the box ranges, euler_view_text against the Python formatter, and the library's new symbols."""
import re

import numpy as np
import pytest

import euler_amd as ea
import overview_ref as ref
import viewport_ref as vref

EULER_EINVAL = -1
GX, GY = 37, 23


def random_state(seed, shape):
    rng = np.random.default_rng(seed)
    solid = (rng.random(shape) < 0.2).astype(np.uint8)
    sink = (rng.random(shape) < 0.15).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.6, rng.integers(0, 9, shape), 0).astype(np.uint8)
    u, v = (rng.standard_normal(shape).astype(np.float32) * 3 for _ in range(2))
    dye = tuple(rng.random(shape, dtype=np.float32) for _ in range(3))
    return solid, sink, count, u, v, dye


def random_markers(rng, box, n=600):
    """markers all over a 37 x 23 grid (and beyond it), with the edges of the box planted: exactly on x0 and on x1 + 1, one float below each, the same
    along y, and non-finite ones"""
    x0, y0, x1, y1 = box
    m = np.empty((n, 2), np.float32)
    m[:, 0] = rng.uniform(-1, GX + 1, n)
    m[:, 1] = rng.uniform(-1, GY + 1, n)
    f = np.float32
    below = lambda a: np.nextafter(f(a), f(-np.inf))
    midx, midy = f(x0 + 0.5), f(y0 + 0.5)
    planted = [(f(x0), midy), (below(x0), midy), (f(x1 + 1), midy), (below(x1 + 1), midy),
               (midx, f(y0)), (midx, below(y0)), (midx, f(y1 + 1)), (midx, below(y1 + 1)),
               (f(x0), f(y0)), (below(x1 + 1), below(y1 + 1)),
               (np.nan, midy), (midx, np.nan), (np.inf, midy), (midx, -np.inf), (np.nan, np.nan)]
    return np.concatenate([m, np.array(planted, np.float32)])


def random_box(rng, X=GX, Y=GY):
    xs, ys = np.sort(rng.integers(1, X - 1, 2)), np.sort(rng.integers(1, Y - 1, 2))
    return int(xs[0]), int(ys[0]), int(xs[1]), int(ys[1])


@pytest.mark.parametrize("seed", range(6))
def test_raster_restatement_against_the_loop(seed):
    rng = np.random.default_rng(100 + seed)
    box = random_box(rng) if seed else (1, 1, GX - 2, GY - 2)
    m = random_markers(rng, box)
    x0, y0, x1, y1 = box
    for scale in vref.SCALES:
        a, b = vref.raster_ref(m, box, scale), vref.raster_loop(m, box, scale)
        assert a.shape == ((y1 - y0 + 1) * scale, (x1 - x0 + 1) * scale) and a.dtype == np.uint32
        assert np.array_equal(a, b), (box, scale)
        # every scale refines scale 1
        assert np.array_equal(a.reshape(y1 - y0 + 1, scale, x1 - x0 + 1, scale).sum(axis=(1, 3)), vref.raster_ref(m, box, 1))
    # the planted ones: on x0 in, just below out, on x1 + 1 out, just below in (column 0 / the last column of the box's middle row ... at least those)
    one = vref.raster_ref(m[-15:], box, 1)
    assert int(one.sum()) == 6      # (x0, mid), (below x1 + 1, mid), (mid, y0), (mid, below y1 + 1) and the two corners
    assert one[-1, 0] >= 1 and one[0, -1] >= 1


@pytest.mark.parametrize("seed", range(4))
def test_box_overview_restatement_against_a_loop(seed):
    rng = np.random.default_rng(200 + seed)
    st = random_state(300 + seed, (GY, GX))
    solid, sink, count, u, v, dye = st
    box = random_box(rng)
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    W, H = int(rng.integers(1, bw + 1)), int(rng.integers(1, bh + 1))
    got = vref.overview_box_ref(*st, box, W, H)
    cols, rows = vref.column_ranges(x0, bw, W), vref.row_ranges(y1, bh, H)
    for py, (yt, yb) in enumerate(rows):
        for px, (xa, xb) in enumerate(cols):
            cells = so = si = wa = marks = 0
            best = np.float32(0)
            d = [0, 0, 0]
            for y in range(yt, yb - 1, -1):
                for x in range(xa, xb + 1):
                    cells += 1
                    if solid[y, x]:
                        so += 1
                    elif sink[y, x]:
                        si += 1
                    elif count[y, x]:
                        wa += 1
                        marks += min(int(count[y, x]), 3)
                        dx = (u[y, x] + u[y, x - 1]) / np.float32(2)
                        dy = (v[y, x] + v[y - 1, x]) / np.float32(2)
                        best = max(best, np.float32(dx * dx + dy * dy))
                        for c in range(3):
                            d[c] += int(ref.q24(dye[c][y, x]))
            r = got[py, px]
            assert (int(r["cells"]), int(r["solid"]), int(r["sink"]), int(r["water"]), int(r["marks"])) == (cells, so, si, wa, marks), (box, W, H, px, py)
            assert r["max_speed2"].view(np.uint32) == best.view(np.uint32) and [int(t) for t in r["dye"]] == d
    # the whole interior is overview_ref itself
    assert not ref.mismatches(vref.overview_box_ref(*st, (1, 1, GX - 2, GY - 2), 7, 5), ref.overview_ref(*st, 7, 5))


def test_box_ranges_tile_the_box():
    rng = np.random.default_rng(7)
    for _ in range(300):
        b = int(rng.integers(1, 5000))
        w = int(rng.integers(1, b + 1))
        lo = int(rng.integers(1, 9000))
        cols = vref.column_ranges(lo, b, w)
        assert cols[0][0] == lo and cols[-1][1] == lo + b - 1
        assert all(a <= z for a, z in cols) and all(cols[k + 1][0] == cols[k][1] + 1 for k in range(w - 1))
        hi = lo + b - 1
        rows = vref.row_ranges(hi, b, w)
        assert rows[0][0] == hi and rows[-1][1] == lo
        assert all(t >= z for t, z in rows) and all(rows[k + 1][0] == rows[k][1] - 1 for k in range(w - 1))
    # the whole interior: euler_overview's own ranges (x = 1 + floor(px Xi / W) ... floor((px + 1) Xi / W); y = Y - 2 - floor(py Yi / H) down to Y - 1 - floor((py + 1) Yi / H))
    Xi, Yi, W, H = 998, 698, 80, 24
    assert vref.column_ranges(1, Xi, W) == [(1 + px * Xi // W, (px + 1) * Xi // W) for px in range(W)]
    assert vref.row_ranges(Yi, Yi, H) == [(Yi - py * Yi // H, Yi + 1 - (py + 1) * Yi // H) for py in range(H)]


def _view_case(seed):
    rng = np.random.default_rng(400 + seed)
    st = random_state(500 + seed, (GY, GX))
    box = random_box(rng)
    x0, y0, x1, y1 = box
    cells = vref.overview_box_ref(*st, box, x1 - x0 + 1, y1 - y0 + 1)
    return cells, box, random_markers(rng, box, 2500)


@pytest.mark.parametrize("rainbow", [False, True])
@pytest.mark.parametrize("scale", [1, 4])
def test_view_text_against_the_python_formatter(scale, rainbow):
    for seed in range(3):
        cells, box, m = _view_case(seed)
        raster = vref.raster_ref(m, box, scale)
        solid, sink, count, rgb = vref.view_grids(cells, raster, scale)
        h, w = raster.shape
        want = ea.render_grids(solid, sink, count, w, h, rgb=rgb if rainbow else None)
        got = ea.view_text(cells, raster, scale, rainbow=rainbow)
        assert got == want, (seed, scale, rainbow)
        rows = re.sub(rb"\x1b\[[0-9;]*[mK]", b"", got).split(b"\r\n")
        assert len(rows) == h and all(len(r) == w for r in rows)
        # glyph by glyph: the class of the cell, else min(3, count of the sub-pixel)
        k = np.repeat(np.repeat(ref.class_ref(cells), scale, axis=0), scale, axis=1)
        table = np.frombuffer(b" oO0", np.uint8)
        want_glyphs = np.where(k == 4, ord("X"), np.where(k == 5, ord("="), table[np.minimum(raster, 3)]))
        assert np.array_equal(np.array([list(r) for r in rows]), want_glyphs)
        if rainbow:
            assert b"\x1b[38;2;" in got
    # at scale 1 with the counts themselves as the raster: the text of the records at one cell per pixel
    st = random_state(9, (GY, GX))
    cells = vref.overview_box_ref(*st, (1, 1, GX - 2, GY - 2), GX - 2, GY - 2)
    raster = np.where(ref.class_ref(cells) < 4, st[2][GY - 2:0:-1, 1:GX - 1], 0).astype(np.uint32)
    assert ea.view_text(cells, raster, 1) == ea.overview_text(cells)


def test_view_text_refusals_and_sizing():
    cells, box, m = _view_case(0)
    bh, bw = cells.shape
    raster = vref.raster_ref(m, box, 2)
    L = ea.load_library()
    n = ea.C.c_int32(0)
    call = lambda c, r, w, h, s, out=None, cap=0: L.euler_view_text(c, r, w, h, s, 0, out, cap, ea.C.byref(n))
    assert call(cells.ctypes.data, raster.ctypes.data, bw, bh, 2) == 0 and n.value > 0
    full = ea.view_text(cells, raster, 2)
    assert len(full) == n.value
    buf = ea.C.create_string_buffer(b"#" * 64, 64)
    assert call(cells.ctypes.data, raster.ctypes.data, bw, bh, 2, buf, 16) == 0 and n.value == len(full)
    assert buf.raw[:16] == full[:16] and buf.raw[16:] == b"#" * 48
    for scale in (0, 3, 5, 32, -1):
        assert call(cells.ctypes.data, raster.ctypes.data, bw, bh, scale) == EULER_EINVAL, scale
    assert call(None, raster.ctypes.data, bw, bh, 2) == EULER_EINVAL and call(cells.ctypes.data, None, bw, bh, 2) == EULER_EINVAL
    assert call(cells.ctypes.data, raster.ctypes.data, 0, bh, 2) == EULER_EINVAL and call(cells.ctypes.data, raster.ctypes.data, bw, 0, 2) == EULER_EINVAL
    assert call(cells.ctypes.data, raster.ctypes.data, 4096, 4096, 2) == EULER_EINVAL      # more than 2^24 glyphs: refused before anything is read
    with pytest.raises(ValueError):
        ea.view_text(cells, raster, 4)


def test_view_zoom_rule_and_keys():
    assert vref.view_zoom(98, 38, 98, 38) == 0 and vref.view_zoom(49, 19, 98, 38) == 2 and vref.view_zoom(49, 20, 98, 38) == 0
    assert vref.view_zoom(4, 4, 200, 50) == 8 and vref.view_zoom(4, 2, 200, 50) == 16 and vref.view_zoom(1, 1, 1000, 1000) == 16
    xi, yi = 98, 38
    box = (1, 1, xi, yi)
    for key in "+++++++":
        box = vref.view_key(box, key, xi, yi)
    assert (box[2] - box[0] + 1, box[3] - box[1] + 1) == (4, 4)      # 98 -> 49 -> 24 -> 12 -> 6 -> 4 (never below), 38 -> 19 -> 9 -> 4
    rng = np.random.default_rng(3)
    for _ in range(500):
        box = vref.view_key(box, "hjkl+-0"[int(rng.integers(0, 7))] if rng.random() < 0.97 else "x", xi, yi)
        assert 1 <= box[0] <= box[2] <= xi and 1 <= box[1] <= box[3] <= yi
    assert vref.view_key((10, 10, 29, 19), "l", xi, yi) == (15, 10, 34, 19) and vref.view_key((10, 10, 29, 19), "j", xi, yi) == (10, 8, 29, 17)
    assert vref.view_key((90, 30, 98, 38), "l", xi, yi) == (90, 30, 98, 38) and vref.view_key((1, 1, 98, 38), "-", xi, yi) == (1, 1, 98, 38)
    assert vref.view_key((10, 10, 29, 19), "-", xi, yi) == (1, 5, 40, 24) and vref.view_key((3, 3, 5, 5), "+", xi, yi) == (3, 3, 5, 5)


def test_library_exports_the_viewport():
    L = ea.load_library()
    for name in ("euler_overview_box", "euler_marker_raster", "euler_view_text", "euler_render_view"):
        assert name in ea.EXPORTS and hasattr(L, name), name
    for name in ("overview", "marker_raster", "render_view"):
        assert hasattr(ea.Simulation, name)
    assert L.euler_abi_version() == 2
