"""Numpy restatement of the flow diagnostics (include/euler.h euler_diag, docs/diagnostics.md), written from the record's definition, not from
the kernel: the yardstick of test_diagnostics_host.py and test_gpu_diagnostics.py.

cell_terms() forms every cell's contribution once (float32 in the stated operation order, the quantisation through an np.float32 multiply
and astype(np.uint64)); reduce_box() sums / maximises them over a box, so many boxes of one state share the work.  diag_loop() is a second,
plain Python-loop restatement for cross-checking the vectorised one.  derive() restates euler_diag_derive in Python doubles.
Test infrastructure only."""
import numpy as np

DTYPE = np.dtype({"names": ["cells", "fluid", "markers", "crowded", "mass_x", "mass_y", "div_l1", "ke_hi", "ke_lo", "count_max", "nonfinite", "max_div", "max_speed2"],
                  "formats": [np.uint64] * 9 + [np.uint32, np.uint32, np.float32, np.float32],
                  "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84], "itemsize": 88})
CROWDED = 8
F32 = np.float32
HEADER = "frame,substeps,pcg_iterations,residual,fluid,markers,count_max,crowded,max_div,mean_abs_div,kinetic_energy,com_x,com_y,nonfinite"


def cell_terms(solid, count, u, v):
    """per cell of the interior (the border ring stays 0): what the cell adds to each sum, and its candidates for the maxima"""
    Y, X = count.shape
    u = np.asarray(u, F32); v = np.asarray(v, F32)
    inner = (slice(1, Y - 1), slice(1, X - 1))
    fl = np.zeros((Y, X), bool)
    fl[inner] = (count[inner] > 0) & (solid[inner] == 0)
    d = np.zeros((Y, X), F32); s2 = np.zeros((Y, X), F32)
    with np.errstate(all="ignore"):
        uc, ul, vc, vb = u[1:Y - 1, 1:X - 1], u[1:Y - 1, 0:X - 2], v[1:Y - 1, 1:X - 1], v[0:Y - 2, 1:X - 1]
        d[inner] = ((uc - ul) + vc) - vb
        dx = (uc + ul) / F32(2)
        dy = (vc + vb) / F32(2)
        s2[inner] = dx * dx + dy * dy
        ad = np.abs(d)
        d_ok, s_ok = fl & ~np.isnan(d), fl & ~np.isnan(s2)
        ad = np.where(d_ok, ad, F32(0)).astype(F32)
        s2 = np.where(s_ok, s2, F32(0)).astype(F32)
        qd = (np.where(ad < F32(256), ad, F32(256)).astype(F32) * F32(16777216.0)).astype(np.uint64)
        qk = (np.where(s2 < F32(16777216.0), s2, F32(16777216.0)).astype(F32) * F32(4294967296.0)).astype(np.uint64)
    cn = np.where(fl, count, 0).astype(np.uint64)
    xs = np.arange(X, dtype=np.uint64)[None, :]
    ys = np.arange(Y, dtype=np.uint64)[:, None]
    return {"fluid": fl, "count": cn, "crowded": fl & (count >= CROWDED), "mass_x": cn * xs, "mass_y": cn * ys,
            "qd": qd, "ke_hi": qk >> np.uint64(32), "ke_lo": qk & np.uint64(0xffffffff),
            "nonfinite": fl & ~(d_ok & s_ok), "ad": ad, "s2": s2}


def reduce_box(t, box=None):
    Y, X = t["fluid"].shape
    x0, y0, x1, y1 = (1, 1, X - 2, Y - 2) if box is None else box
    assert 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= Y - 2
    b = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    r = np.zeros((), DTYPE)
    r["cells"] = (x1 - x0 + 1) * (y1 - y0 + 1)
    for name, key in (("fluid", "fluid"), ("markers", "count"), ("crowded", "crowded"), ("mass_x", "mass_x"), ("mass_y", "mass_y"), ("div_l1", "qd"),
                      ("ke_hi", "ke_hi"), ("ke_lo", "ke_lo"), ("nonfinite", "nonfinite")):
        r[name] = int(t[key][b].sum(dtype=np.uint64))
    r["count_max"] = int(t["count"][b].max())
    r["max_div"] = t["ad"][b].max()          # (non-negative, NaNs already 0: the float maximum is the maximum of the bit patterns)
    r["max_speed2"] = t["s2"][b].max()
    return r


def diag_ref(solid, count, u, v, box=None):
    return reduce_box(cell_terms(solid, count, u, v), box)


def diag_loop(solid, count, u, v, box=None):
    """the same record by one Python loop over the cells of the box, scalar np.float32 arithmetic"""
    Y, X = count.shape
    x0, y0, x1, y1 = (1, 1, X - 2, Y - 2) if box is None else box
    acc = {n: 0 for n in DTYPE.names}
    acc["cells"] = (x1 - x0 + 1) * (y1 - y0 + 1)
    maxd = maxs = 0      # unsigned bit patterns
    with np.errstate(all="ignore"):
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                c = int(count[y, x])
                if c == 0 or solid[y, x]:
                    continue
                acc["fluid"] += 1; acc["markers"] += c; acc["crowded"] += c >= CROWDED
                acc["mass_x"] += c * x; acc["mass_y"] += c * y
                acc["count_max"] = max(acc["count_max"], c)
                ui, ul, vi, vb = F32(u[y, x]), F32(u[y, x - 1]), F32(v[y, x]), F32(v[y - 1, x])
                d = F32(F32(F32(ui - ul) + vi) - vb)
                dx, dy = F32(F32(ui + ul) / F32(2)), F32(F32(vi + vb) / F32(2))
                s2 = F32(F32(dx * dx) + F32(dy * dy))
                if not np.isnan(d):
                    a = F32(abs(d))
                    maxd = max(maxd, int(a.view(np.uint32)))
                    acc["div_l1"] += int(np.uint64(F32((a if a < F32(256) else F32(256)) * F32(16777216.0))))
                if not np.isnan(s2):
                    maxs = max(maxs, int(s2.view(np.uint32)))
                    q = int(np.uint64(F32((s2 if s2 < F32(16777216.0) else F32(16777216.0)) * F32(4294967296.0))))
                    acc["ke_hi"] += q >> 32; acc["ke_lo"] += q & 0xffffffff
                acc["nonfinite"] += bool(np.isnan(d) or np.isnan(s2))
    r = np.zeros((), DTYPE)
    for n in DTYPE.names[:11]:
        r[n] = acc[n]
    r["max_div"] = np.uint32(maxd).view(F32)
    r["max_speed2"] = np.uint32(maxs).view(F32)
    return r


def derive(r):
    """euler_diag_derive in Python doubles"""
    fluid, markers = int(r["fluid"]), int(r["markers"])
    if fluid == 0:
        return dict.fromkeys(("mean_abs_div", "kinetic_energy", "com_x", "com_y", "markers_per_cell", "crowded_fraction"), 0.0)
    return {"mean_abs_div": float(int(r["div_l1"])) / 16777216.0 / float(fluid), "kinetic_energy": 0.5 * (float(int(r["ke_hi"])) + float(int(r["ke_lo"])) / 4294967296.0),
            "com_x": float(int(r["mass_x"])) / float(markers), "com_y": float(int(r["mass_y"])) / float(markers),
            "markers_per_cell": float(markers) / float(fluid), "crowded_fraction": float(int(r["crowded"])) / float(fluid)}


def mismatches(got, want):
    """names of the record fields that differ; the two floats are compared as bits"""
    bad = []
    for n in DTYPE.names:
        a, b = np.asarray(got[n]).reshape(1), np.asarray(want[n]).reshape(1)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.astype(np.float32).view(np.uint32)
        if int(a[0]) != int(b[0]):
            bad.append("%s: %s != %s" % (n, got[n], want[n]))
    return bad


def boxes(X, Y, seed, n=20):
    """the boxes every grid is checked with: the whole interior, one cell, one row, one column, and n seeded random ones - among them boxes whose left
    edge cuts a group of four cells (x0 % 4 != 0) and whose right edge does (x1 % 4 != 3), a box inside one 64 x 64 tile where the grid has room, and one
    that spans several tiles"""
    rng = np.random.default_rng(seed)
    out = [None, (X // 2, Y // 2, X // 2, Y // 2), (1, Y // 3, X - 2, Y // 3), (X // 3, 1, X // 3, Y - 2)]
    for k in range(n):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya, yb = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
        if k == 0 and X > 70 and Y > 70:      # inside one tile
            xa, xb, ya, yb = 66, 70, 65, 69
        if k == 1:
            xa, xb = min(5, X - 2), max(X - 4, min(5, X - 2))      # several tiles, both edges cut (5 % 4 = 1)
        out.append((xa, ya, xb, yb))
    assert any(b[0] % 4 != 0 for b in out[1:]) and any(b[2] % 4 != 3 for b in out[1:])
    return out


def csv_line(frame, stats, r):
    """the line `euler --stats` writes for a frame (floats as C's %.9g)"""
    v = derive(r)
    g = lambda x: "%.9g" % x
    return ",".join([str(frame), str(stats.last_substeps), str(stats.last_pcg_iterations), g(stats.last_residual), str(int(r["fluid"])), str(int(r["markers"])),
                     str(int(r["count_max"])), str(int(r["crowded"])), g(float(r["max_div"])), g(v["mean_abs_div"]), g(v["kinetic_energy"]), g(v["com_x"]), g(v["com_y"]),
                     str(int(r["nonfinite"]))])
