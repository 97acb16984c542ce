"""Numpy restatement of the flow raster (include/euler.h euler_flow_px, docs/flow_raster.md) and of euler_flow_paint, written from the record's
definition, not from the kernel: the yardstick of test_flow_host.py and test_gpu_flow.py.

Box edges by the integer formulas, sums by np.add.reduceat in uint64, the terms in float32 in the stated operation order, maxima by
np.maximum.reduceat with the NaNs replaced by 0 first.  It works on the arrays euler_get_field returns.  Test infrastructure only."""
import numpy as np

from overview_ref import _boxes, edges

DTYPE = np.dtype({"names": ["cells", "water", "nodes", "nonfinite", "u_pos", "u_neg", "v_pos", "v_neg", "w_pos", "w_neg", "p_sum", "max_speed2", "max_abs_w", "max_p", "reserved"],
                  "formats": [np.uint32] * 4 + [np.uint64] * 7 + [np.float32] * 3 + [np.uint32],
                  "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84], "itemsize": 88})
FLOATS = ("max_speed2", "max_abs_w", "max_p")
VORTICITY, PRESSURE, SPEED = 0, 1, 2
F2 = np.float32(2)


def qv(a):
    """a >= 0, no NaN: 2^-20 units, saturating at 2^12"""
    a = np.asarray(a, np.float32)
    return (np.where(a < np.float32(4096), a, np.float32(4096)).astype(np.float32) * np.float32(1048576)).astype(np.uint64)


def qp(a):
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(a > 0, np.where(a < np.float32(16777216), a, np.float32(16777216)), np.float32(0)).astype(np.float32)      # (a NaN fails a > 0)
    return (c * np.float32(256)).astype(np.uint64)


def _signed(a, valid):
    """(terms of the positive side, terms of the negative side) of a where valid and not a NaN; -0.0 >= 0"""
    ok = valid & ~np.isnan(a)
    a = np.where(ok, a, np.float32(0)).astype(np.float32)
    pos, neg = ok & (a >= 0), ok & (a < 0)
    return np.where(pos, qv(np.where(pos, a, 0)), 0).astype(np.uint64), np.where(neg, qv(np.where(neg, -a, 0)), 0).astype(np.uint64)


def cell_terms(solid, sink, count, u, v, p=None):
    """the per-cell terms over the whole interior, index [y - 1, x - 1]"""
    Y, X = count.shape
    u = np.asarray(u, np.float32); v = np.asarray(v, np.float32)
    wat = (np.asarray(solid) == 0) & (np.asarray(sink) == 0) & (np.asarray(count) > 0)
    c = (slice(1, Y - 1), slice(1, X - 1))
    with np.errstate(all="ignore"):
        dx = ((u[c] + u[1:Y - 1, 0:X - 2]) / F2).astype(np.float32)
        dy = ((v[c] + v[0:Y - 2, 1:X - 1]) / F2).astype(np.float32)
        s2 = (dx * dx + dy * dy).astype(np.float32)
        w = ((v[1:Y - 1, 2:X] - v[c]) - (u[2:Y, 1:X - 1] - u[c])).astype(np.float32)
    water = wat[c]
    wet = water & wat[1:Y - 1, 2:X] & wat[2:Y, 1:X - 1] & wat[2:Y, 2:X]
    t = {"water": water, "nodes": wet & ~np.isnan(w)}
    t["u_pos"], t["u_neg"] = _signed(dx, water)
    t["v_pos"], t["v_neg"] = _signed(dy, water)
    t["w_pos"], t["w_neg"] = _signed(w, wet)
    bad = water & (np.isnan(dx) | np.isnan(dy) | (wet & np.isnan(w)))
    t["max_speed2"] = np.where(water & ~np.isnan(s2), s2, np.float32(0)).astype(np.float32)
    t["max_abs_w"] = np.where(t["nodes"], np.abs(w), np.float32(0)).astype(np.float32)
    if p is not None:
        with np.errstate(all="ignore"):
            pf = np.asarray(p, np.float64)[c].astype(np.float32)
        bad = bad | (water & np.isnan(pf))
        t["p_sum"] = np.where(water, qp(pf), 0).astype(np.uint64)
        with np.errstate(invalid="ignore"):
            t["max_p"] = np.where(water & (pf > 0), pf, np.float32(0)).astype(np.float32)
    t["nonfinite"] = bad
    return t


def reduce_box(terms, box, W, H):
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    assert 1 <= W <= bw and 1 <= H <= bh
    xs, ys = edges(bw, W), edges(bh, H)
    out = np.zeros((H, W), DTYPE)
    out["cells"] = np.outer(np.diff(np.append(ys, bh)), np.diff(np.append(xs, bw)))
    for n, a in terms.items():
        a = a[y0 - 1:y1, x0 - 1:x1][::-1]      # the box, its top row first
        if n in FLOATS:
            out[n] = _boxes(a, xs, ys, np.maximum, np.float32)
        else:
            out[n] = _boxes(a.astype(np.uint64), xs, ys)
    return out


def flow_ref(solid, sink, count, u, v, box, W, H, p=None):
    """All grids (Y, X) as euler_get_field returns them; p: EULER_F_PRESSURE for EULER_FLOW_PRESSURE, else None."""
    return reduce_box(cell_terms(solid, sink, count, u, v, p), box, W, H)


def mismatches(got, want):
    """names of the record fields that differ; the maxima are compared as bits"""
    bad = []
    for n in DTYPE.names:
        a, b = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])
        if n in FLOATS:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append(n)
    return bad


def q24(x):
    x = np.asarray(x, np.float32)
    c = np.where(x > 0, np.minimum(x, np.float32(1)), np.float32(0)).astype(np.float32)
    return (c * np.float32(16777216.0)).astype(np.uint64)


def paint_ref(flow, px, field, scale):
    """euler_flow_paint: a painted copy of px (doubles throughout, the colour narrowed to float32 in front of q24)"""
    out = px.copy()
    water = flow["water"].astype(np.float64)
    wdiv = np.maximum(water, 1)
    sub = lambda a, b: flow[a].astype(np.float64) - flow[b].astype(np.float64)
    if field == VORTICITY:
        nodes = flow["nodes"].astype(np.float64)
        m = np.where(nodes > 0, sub("w_pos", "w_neg") / 1048576.0 / np.maximum(nodes, 1), 0.0)
        t = np.clip(m / scale, -1.0, 1.0)
        lin = np.where(t[..., None] >= 0, np.stack([np.ones_like(t), 1 - t, 1 - t], -1), np.stack([1 + t, 1 + t, np.ones_like(t)], -1))
    else:
        if field == PRESSURE:
            m = flow["p_sum"].astype(np.float64) / 256.0 / wdiv
        else:
            mu, mv = sub("u_pos", "u_neg") / 1048576.0 / wdiv, sub("v_pos", "v_neg") / 1048576.0 / wdiv
            m = np.sqrt(mu * mu + mv * mv)
        t = np.clip(np.where(water > 0, m, 0.0) / scale, 0.0, 1.0)
        lin = np.stack([t, np.full_like(t, 0.5), 1 - t], -1)
    out["dye"] = flow["water"].astype(np.uint64)[..., None] * q24(lin.astype(np.float32))
    return out
