"""Numpy restatement of the whole-domain overview (include/euler.h euler_overview_px, docs/overview.md), written from the record's
definition and the formatters' rules, not from the kernel: the yardstick of test_overview_host.py and test_gpu_overview.py.

Box edges by the integer formulas, sums by np.add.reduceat in uint64, max_speed2 in float32 in the expression's operation order
(np.maximum.reduceat, NaNs replaced by 0 first).  Test infrastructure only."""
import numpy as np

DTYPE = np.dtype({"names": ["cells", "solid", "sink", "water", "marks", "max_speed2", "dye"],
                  "formats": [np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.float32, (np.uint64, 3)],
                  "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 48})
COVERAGE, DYE, SPEED = 0, 1, 2


def edges(n_cells, n_px):
    """starts of the boxes along one axis, as 0-based interior offsets: floor(p * n_cells / n_px), p = 0 .. n_px - 1 (Python integers)"""
    return np.array([p * n_cells // n_px for p in range(n_px)], np.intp)


def _boxes(a, xs, ys, op=np.add, dtype=np.uint64):
    """a: (Yi, Xi) with row 0 = the TOP interior row; reduce over the boxes (sums in uint64 whatever a's type)"""
    return op.reduceat(op.reduceat(a, ys, axis=0, dtype=dtype), xs, axis=1, dtype=dtype)


def q24(x):
    x = np.asarray(x, np.float32)
    c = np.where(x > 0, np.minimum(x, np.float32(1)), np.float32(0)).astype(np.float32)      # (a NaN fails x > 0)
    return (c * np.float32(16777216.0)).astype(np.uint64)


def overview_ref(solid, sink, count, u, v, dye, W, H):
    """dye: None or (r, g, b).  All grids (Y, X) as euler_get_field returns them."""
    Y, X = count.shape
    Xi, Yi = X - 2, Y - 2
    assert 1 <= W <= Xi and 1 <= H <= Yi
    xs, ys = edges(Xi, W), edges(Yi, H)
    inner = (slice(Y - 2, 0, -1), slice(1, X - 1))      # rows Y-2 .. 1 (top first), columns 1 .. X-2
    so = solid[inner] != 0
    si = ~so & (sink[inner] != 0)
    cn = count[inner]
    wa = ~so & ~si & (cn > 0)
    out = np.zeros((H, W), DTYPE)
    out["cells"] = np.outer(np.diff(np.append(ys, Yi)), np.diff(np.append(xs, Xi)))
    out["solid"] = _boxes(so, xs, ys)
    out["sink"] = _boxes(si, xs, ys)
    out["water"] = _boxes(wa, xs, ys)
    out["marks"] = _boxes(np.where(wa, np.minimum(cn, 3), 0).astype(np.uint8), xs, ys)
    u = np.asarray(u, np.float32); v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        dx = (u[Y - 2:0:-1, 1:X - 1] + u[Y - 2:0:-1, 0:X - 2]) / np.float32(2)
        dy = (v[Y - 2:0:-1, 1:X - 1] + v[Y - 3::-1, 1:X - 1]) / np.float32(2)
        s2 = (dx * dx + dy * dy).astype(np.float32)
    s2 = np.where(wa & ~np.isnan(s2), s2, np.float32(0)).astype(np.float32)
    out["max_speed2"] = _boxes(s2, xs, ys, np.maximum, np.float32)
    if dye is not None:
        for c in range(3):
            out["dye"][..., c] = _boxes(np.where(wa, q24(dye[c][inner]), 0).astype(np.uint32), xs, ys)
    return out


def class_ref(px):
    """per record: 0 air, 1..3 the glyph index, 4 solid, 5 sink"""
    cells, solid, sink, marks = (px[n].astype(np.int64) for n in ("cells", "solid", "sink", "marks"))
    open_ = cells - solid - sink
    k = np.minimum(3, (marks + open_ - 1) // np.maximum(open_, 1))
    return np.where(2 * solid >= cells, 4, np.where((sink > 0) & (sink >= open_), 5, k))


def mean_dye(px):
    w = px["water"].astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        return np.where(w > 0, px["dye"].astype(np.float64) / (np.maximum(w, 1) * 16777216.0), 0.0).astype(np.float32)


def srgb_bytes(lin):
    end = np.nextafter(np.float32(256), np.float32(0))
    v = end * np.power(np.asarray(lin, np.float32), np.float32(1 / 2.2), dtype=np.float32)
    return np.clip(v, np.float32(0), end).astype(np.int64)


def rgb_ref(px, mode, scale=1.0):
    h, w = px.shape
    wc = np.empty((h, w, 3), np.int64)
    if mode == COVERAGE:
        wc[...] = (64, 128, 255)
    elif mode == DYE:
        wc[...] = srgb_bytes(mean_dye(px))
    else:
        with np.errstate(all="ignore"):
            t = np.minimum(np.float32(1), np.sqrt(px["max_speed2"], dtype=np.float32) / np.float32(scale)).astype(np.float32)
        wc[..., 0] = (np.float32(255) * t + np.float32(0.5)).astype(np.int64)
        wc[..., 1] = 128
        wc[..., 2] = (np.float32(255) * (np.float32(1) - t) + np.float32(0.5)).astype(np.int64)
    cells, solid, sink, water = (px[n].astype(np.int64)[..., None] for n in ("cells", "solid", "sink", "water"))
    return ((solid * 128 + sink * 64 + water * wc + cells // 2) // cells).astype(np.uint8)


def mismatches(got, want):
    """names of the record fields that differ; max_speed2 is compared as bits"""
    bad = []
    for n in DTYPE.names:
        a, b = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])
        if n == "max_speed2":
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append(n)
    return bad
