"""Numpy restatement of the pan-and-zoom viewport (include/euler.h euler_overview_box / euler_marker_raster / euler_view_text,
docs/viewport.md), written from the definitions, not from the kernels: the yardstick of test_viewport_host.py and test_gpu_viewport.py.

The box overview is overview_ref.py's reduction over the box with one ring of cells around it (the ring is what u[i-1] and v[i-X] of the
box's first column and bottom row read).  The raster is float32 arithmetic as the definition states it, with a plain Python-loop twin
in exact arithmetic (a float32 is a double; the difference and the product by a power of two are exact in doubles).  The magnified frame is
the classes and counts repeated scale x scale and handed to the frame formatter that the golden frames pin.  Test infrastructure only."""
import math

import numpy as np

import overview_ref as ref

SCALES = (1, 2, 4, 8, 16)


def column_ranges(x0, bw, w):
    """[(first, last)] of the cells of pixel columns 0 .. w - 1: x0 + floor(px bw / w) ... x0 + floor((px + 1) bw / w) - 1 (Python integers)"""
    return [(x0 + px * bw // w, x0 + (px + 1) * bw // w - 1) for px in range(w)]


def row_ranges(y1, bh, h):
    """[(top, bottom)] of pixel rows 0 .. h - 1, row 0 = the top: y1 - floor(py bh / h) down to y1 + 1 - floor((py + 1) bh / h)"""
    return [(y1 - py * bh // h, y1 + 1 - (py + 1) * bh // h) for py in range(h)]


def overview_box_ref(solid, sink, count, u, v, dye, box, W, H):
    """dye: None or (r, g, b); all grids (Y, X); box = (x0, y0, x1, y1) inclusive, inside the interior"""
    x0, y0, x1, y1 = box
    Y, X = count.shape
    assert 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= Y - 2
    cut = (slice(y0 - 1, y1 + 2), slice(x0 - 1, x1 + 2))
    return ref.overview_ref(solid[cut], sink[cut], count[cut], u[cut], v[cut], None if dye is None else tuple(d[cut] for d in dye), W, H)


def raster_ref(markers, box, scale):
    """uint32 (Bh scale, Bw scale), row 0 = top: markers per sub-pixel"""
    x0, y0, x1, y1 = box
    W, H = (x1 - x0 + 1) * scale, (y1 - y0 + 1) * scale
    m = np.ascontiguousarray(markers, np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        sx = ((m[:, 0] - np.float32(x0)) * np.float32(scale)).astype(np.float32)
        sy = ((m[:, 1] - np.float32(y0)) * np.float32(scale)).astype(np.float32)
        ok = np.isfinite(m).all(axis=1) & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    c = np.floor(sx[ok]).astype(np.int64)
    r = H - 1 - np.floor(sy[ok]).astype(np.int64)
    return np.bincount(r * W + c, minlength=W * H).astype(np.uint32).reshape(H, W)


def raster_loop(markers, box, scale):
    """the same, marker by marker in exact arithmetic"""
    x0, y0, x1, y1 = box
    W, H = (x1 - x0 + 1) * scale, (y1 - y0 + 1) * scale
    out = np.zeros((H, W), np.uint32)
    for mx, my in np.ascontiguousarray(markers, np.float32).reshape(-1, 2).tolist():
        if not (math.isfinite(mx) and math.isfinite(my)):
            continue
        c, k = math.floor((mx - x0) * scale), math.floor((my - y0) * scale)
        if 0 <= c < W and 0 <= k < H:
            out[H - 1 - k, c] += 1
    return out


def view_grids(cells, raster, scale):
    """(solid, sink, count, (r, g, b)) of the (Bh scale + 2, Bw scale + 2) grid whose frame is the magnified view: row index = y as the frame
    formatter reads it (row 0 = the bottom border), a ring of nothing around"""
    bh, bw = cells.shape
    assert raster.shape == (bh * scale, bw * scale)
    up = lambda a: np.repeat(np.repeat(a, scale, axis=0), scale, axis=1)
    k = up(ref.class_ref(cells))
    dye = ref.mean_dye(cells)
    grids = [np.zeros((bh * scale + 2, bw * scale + 2), t) for t in (np.uint8, np.uint8, np.uint8, np.float32, np.float32, np.float32)]
    inner = (slice(bh * scale, 0, -1), slice(1, bw * scale + 1))      # picture row 0 = grid row H
    grids[0][inner] = k == 4
    grids[1][inner] = k == 5
    grids[2][inner] = np.where(k < 4, np.minimum(raster, 3), 0)
    for c in range(3):
        grids[3 + c][inner] = up(dye[..., c])
    return grids[0], grids[1], grids[2], tuple(grids[3:])


def view_zoom(bw, bh, wx, wy):
    """euler_render_view's choice: 0 = boxes of cells (W = min(wx, bw), H = min(wy, bh)), else the scale of the raster"""
    if bw * 2 > wx or bh * 2 > wy:
        return 0
    return max(s for s in SCALES if bw * s <= wx and bh * s <= wy)


# ---- the `euler` front end's --view keys (euler_cli.c view_key) ----
def _zoom_axis(lo, hi, limit, nw):
    w = hi - lo + 1
    l = lo + (w - nw) // 2 if nw < w else lo - (nw - w) // 2
    l = max(1, l)
    if l + nw - 1 > limit:
        l = limit - nw + 1
    return l, l + nw - 1


def view_key(box, key, xi, yi):
    """the box after one key: h j k l pan by a quarter of the box, + halves it about its centre (never below 4 x 4 cells), - doubles it, 0 = the interior"""
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    dx, dy = max(1, bw // 4), max(1, bh // 4)
    if key == "h":
        s = min(dx, x0 - 1); x0 -= s; x1 -= s
    elif key == "l":
        s = min(dx, xi - x1); x0 += s; x1 += s
    elif key == "j":
        s = min(dy, y0 - 1); y0 -= s; y1 -= s
    elif key == "k":
        s = min(dy, yi - y1); y0 += s; y1 += s
    elif key == "+":
        x0, x1 = _zoom_axis(x0, x1, xi, bw // 2 if bw // 2 >= 4 else min(bw, 4))
        y0, y1 = _zoom_axis(y0, y1, yi, bh // 2 if bh // 2 >= 4 else min(bh, 4))
    elif key == "-":
        x0, x1 = _zoom_axis(x0, x1, xi, min(2 * bw, xi))
        y0, y1 = _zoom_axis(y0, y1, yi, min(2 * bh, yi))
    elif key == "0":
        x0, y0, x1, y1 = 1, 1, xi, yi
    return x0, y0, x1, y1
