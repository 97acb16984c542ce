"""Numpy restatement of the batched gauges (include/euler.h euler_gauge_rec, docs/gauges.md), written from the record's definition, not from the kernel:
the yardstick of test_gauges_host.py and test_gpu_gauges.py.

gauge_ref works on the arrays euler_get_field returns - (Y, X), row 0 the bottom - with the terms in float32, the quantisation through an np.float32
multiply and astype(np.uint64), and uint64 sums.  gauge_loop is a second restatement in plain loops over the cells.  derive restates
euler_gauge_derive in Python doubles, csv_line the line `euler --gauges` writes.  Test infrastructure only."""
import numpy as np

LEVEL, PRESSURE, FORCE, FLUX = range(4)
KINDS = ("level", "pressure", "force", "flux")
GAUGE_DTYPE = np.dtype({"names": ["kind", "x0", "y0", "x1", "y1", "reserved"], "formats": [np.int32] * 6, "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 24})
DTYPE = np.dtype({"names": ["cells", "fluid", "lo_x", "hi_x", "lo_y", "hi_y", "terms", "nonfinite", "a_pos", "a_neg", "b_pos", "b_neg", "max_a", "max_b"],
                  "formats": [np.uint32] * 8 + [np.uint64] * 4 + [np.float32] * 2,
                  "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 68], "itemsize": 72})
FLOATS = ("max_a", "max_b")
CSV_HEADER = "frame,gauge,kind,cells,fluid,lo_x,hi_x,lo_y,hi_y,terms,a,b,max_a,max_b,nonfinite\n"
NONE = 0xFFFFFFFF
F0 = np.float32(0)


def qv(a):
    """a >= 0, no NaN: 2^-20 units, saturating at 2^12"""
    a = np.asarray(a, np.float32)
    return (np.where(a < np.float32(4096), a, np.float32(4096)).astype(np.float32) * np.float32(1048576)).astype(np.uint64)


def qp(a):
    """no NaN: 2^-8 units, clamped to [0, 2^24]"""
    a = np.asarray(a, np.float32)
    c = np.where(a > 0, np.where(a < np.float32(16777216), a, np.float32(16777216)), F0).astype(np.float32)
    return (c * np.float32(256)).astype(np.uint64)


def _usum(terms, where):
    return np.uint64(np.where(where, terms, np.uint64(0)).astype(np.uint64).sum(dtype=np.uint64))


def _signed(a, live):
    """(sum of the positive side, of the negative side, max |a|, cells with a NaN) of the float32 terms a where live; -0.0 >= 0"""
    nan = live & np.isnan(a)
    ok = live & ~nan
    z = np.where(ok, a, F0).astype(np.float32)
    pos, neg = ok & (z >= 0), ok & (z < 0)
    mx = np.where(ok, np.abs(z), F0).astype(np.float32).max(initial=F0)
    return _usum(qv(np.where(pos, z, F0)), pos), _usum(qv(np.where(neg, -z, F0)), neg), np.float32(mx), nan


def gauge_ref(solid, count, u, v, p, kind, box):
    """One record (a 0-d array of DTYPE).  p may be None for LEVEL and FLUX."""
    x0, y0, x1, y1 = (int(t) for t in box)
    X = count.shape[1]
    assert 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= count.shape[0] - 2
    sh = lambda a, dy, dx: np.asarray(a)[y0 + dy:y1 + 1 + dy, x0 + dx:x1 + 1 + dx]
    cn, so = sh(count, 0, 0) > 0, sh(solid, 0, 0) != 0
    fluid = cn & ~so
    r = np.zeros((), DTYPE)
    r["cells"] = (x1 - x0 + 1) * (y1 - y0 + 1)
    r["fluid"] = fluid.sum()
    ys, xs = np.nonzero(fluid)
    r["lo_x"], r["hi_x"] = (xs.min() + x0, xs.max() + x0) if len(xs) else (NONE, 0)
    r["lo_y"], r["hi_y"] = (ys.min() + y0, ys.max() + y0) if len(ys) else (NONE, 0)
    if kind in (PRESSURE, FORCE):
        with np.errstate(all="ignore"):
            pf = sh(np.asarray(p, np.float64), 0, 0).astype(np.float32)
        nan = np.isnan(pf)
        q = qp(np.where(nan, F0, pf))
        with np.errstate(invalid="ignore"):
            pm = np.where(~nan & (pf > 0), pf, F0).astype(np.float32)
    if kind == PRESSURE:
        r["terms"] = r["fluid"]
        r["a_pos"] = _usum(q, fluid & ~nan)
        r["max_a"] = np.where(fluid, pm, F0).max(initial=F0)
        r["nonfinite"] = (fluid & nan).sum()
    elif kind == FORCE:
        faces = [fluid & (sh(solid, dy, dx) != 0) for (dy, dx) in ((0, 1), (0, -1), (1, 0), (-1, 0))]      # x+1, x-1, y+1, y-1
        r["terms"] = sum(int(f.sum()) for f in faces)
        for name, f in zip(("a_pos", "a_neg", "b_pos", "b_neg"), faces):
            r[name] = _usum(q, f & ~nan)
        r["max_a"] = np.where(faces[0] | faces[1], pm, F0).max(initial=F0)
        r["max_b"] = np.where(faces[2] | faces[3], pm, F0).max(initial=F0)
        r["nonfinite"] = ((faces[0] | faces[1] | faces[2] | faces[3]) & nan).sum()
    elif kind == FLUX:
        live_u = (cn | (sh(count, 0, 1) > 0)) & ~(so | (sh(solid, 0, 1) != 0))
        live_v = (cn | (sh(count, 1, 0) > 0)) & ~(so | (sh(solid, 1, 0) != 0))
        r["a_pos"], r["a_neg"], r["max_a"], nan_u = _signed(sh(np.asarray(u, np.float32), 0, 0), live_u)
        r["b_pos"], r["b_neg"], r["max_b"], nan_v = _signed(sh(np.asarray(v, np.float32), 0, 0), live_v)
        r["terms"] = int(live_u.sum()) + int(live_v.sum())
        r["nonfinite"] = (nan_u | nan_v).sum()
    else:
        assert kind == LEVEL
    return r


def gauges_ref(solid, count, u, v, p, gauges):
    """the records of a list of (kind, box)"""
    out = np.zeros(len(gauges), DTYPE)
    for k, (kind, box) in enumerate(gauges):
        out[k] = gauge_ref(solid, count, u, v, p, kind, box)
    return out


def _q_scalar(a, clamp, scale):
    """one term, float32 throughout: clamp from above, times a power of two, truncated"""
    a = np.float32(a)
    c = a if a < np.float32(clamp) else np.float32(clamp)
    return int(np.float32(c) * np.float32(scale))


def gauge_loop(solid, count, u, v, p, kind, box):
    """The same record cell by cell, in Python integers."""
    x0, y0, x1, y1 = (int(t) for t in box)
    f = dict(cells=0, fluid=0, lo_x=NONE, hi_x=0, lo_y=NONE, hi_y=0, terms=0, nonfinite=0, a_pos=0, a_neg=0, b_pos=0, b_neg=0)
    mx = {"max_a": F0, "max_b": F0}

    def signed(pos, neg, m, a):
        a = np.float32(a)
        f["terms"] += 1
        if np.isnan(a):
            return True
        if a >= 0:
            f[pos] += _q_scalar(a, 4096, 1048576)
        else:
            f[neg] += _q_scalar(-a, 4096, 1048576)
        mx[m] = max(mx[m], np.float32(abs(a)))
        return False

    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            f["cells"] += 1
            is_fluid = count[y, x] > 0 and not solid[y, x]
            if is_fluid:
                f["fluid"] += 1
                f["lo_x"], f["hi_x"], f["lo_y"], f["hi_y"] = min(f["lo_x"], x), max(f["hi_x"], x), min(f["lo_y"], y), max(f["hi_y"], y)
            if kind == FLUX:
                bad = False
                if (count[y, x] or count[y, x + 1]) and not (solid[y, x] or solid[y, x + 1]):
                    bad |= signed("a_pos", "a_neg", "max_a", u[y, x])
                if (count[y, x] or count[y + 1, x]) and not (solid[y, x] or solid[y + 1, x]):
                    bad |= signed("b_pos", "b_neg", "max_b", v[y, x])
                f["nonfinite"] += int(bad)
            if kind not in (PRESSURE, FORCE) or not is_fluid:
                continue
            with np.errstate(all="ignore"):
                pf = np.float32(np.float64(p[y, x]))
            q = 0 if np.isnan(pf) or not pf > 0 else _q_scalar(pf, 16777216, 256)
            pm = pf if pf > 0 else F0
            if kind == PRESSURE:
                f["terms"] += 1
                if np.isnan(pf):
                    f["nonfinite"] += 1
                else:
                    f["a_pos"] += q
                    mx["max_a"] = max(mx["max_a"], pm)
            else:
                touched = [(n, m) for (n, m, yy, xx) in (("a_pos", "max_a", y, x + 1), ("a_neg", "max_a", y, x - 1), ("b_pos", "max_b", y + 1, x), ("b_neg", "max_b", y - 1, x)) if solid[yy, xx]]
                f["terms"] += len(touched)
                if touched and np.isnan(pf):
                    f["nonfinite"] += 1
                elif touched:
                    for n, m in touched:
                        f[n] += q
                        mx[m] = max(mx[m], pm)
    r = np.zeros((), DTYPE)
    for n, val in f.items():
        r[n] = val
    r["max_a"], r["max_b"] = mx["max_a"], mx["max_b"]
    return r


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


def derive(rec, kind):
    """euler_gauge_derive in Python doubles"""
    out = dict(a=0.0, b=0.0, mean_a=0.0, depth=0.0)
    if int(rec["fluid"]) == 0:
        return out
    scale = 1048576.0 if kind == FLUX else 256.0
    out["a"] = (float(int(rec["a_pos"])) - float(int(rec["a_neg"]))) / scale
    out["b"] = (float(int(rec["b_pos"])) - float(int(rec["b_neg"]))) / scale
    out["mean_a"] = out["a"] / float(int(rec["terms"])) if int(rec["terms"]) else 0.0
    out["depth"] = float(int(rec["hi_y"])) - float(int(rec["lo_y"])) + 1.0
    return out


def csv_line(frame, index, kind, rec):
    """the line `euler --gauges FILE` writes for gauge `index` after frame `frame`"""
    d = derive(rec, kind)
    return "%d,%d,%s,%d,%d,%d,%d,%d,%d,%d,%.9g,%.9g,%.9g,%.9g,%d\n" % (
        frame, index, KINDS[kind], int(rec["cells"]), int(rec["fluid"]), int(rec["lo_x"]), int(rec["hi_x"]), int(rec["lo_y"]), int(rec["hi_y"]), int(rec["terms"]),
        d["a"], d["b"], float(rec["max_a"]), float(rec["max_b"]), int(rec["nonfinite"]))
