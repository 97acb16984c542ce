"""Test-side restatement of the marker density control (euler_set_reseed, include/euler.h, docs/reseed.md): thin crowded cells, refill torn holes.

Written from the header's rule, not from the kernels: the yardstick of test_reseed_host.py and test_gpu_reseed.py.
  reseed           a record as a dict (thin_above, fill_holes, max_cells, max_fill)
  pass_arrays      ONE pass over numpy arrays, vectorised: -> the new marker array and RNG state; count is changed in place, the totals are added to a dict
  pass_loops       the same pass in plain Python loops, literally the header's sentences (a second restatement)
  pass_c           the same pass by euler_host.c's eu_reseed_pass (the library's own sequential reference), in the shape of the two above
  apply            pass_arrays on an oracle, where the pass stands: right behind eo_refresh_marker_counts
  substep / step   eo_substep / eo_step composed over the oracle's exported stage functions as forcing_ref / bodies_ref do, the pass behind the refresh;
                   with every argument at its default and the record off they ARE eo_substep / eo_step (test_reseed_host.py holds them to that)

Test infrastructure only: nothing under euler_amd/ imports this module."""
import ctypes as C

import numpy as np

import euler_amd as ea
import forcing_ref as fref
import heat_ref as href

F32 = np.float32
DEFAULT_LIMIT = 65536
M64 = (1 << 64) - 1
STAT_NAMES = ("removed", "added", "cells_thinned", "deferred")


def reseed(thin_above=0, fill_holes=False, max_cells=0, max_fill=0):
    return dict(thin_above=int(thin_above), fill_holes=int(bool(fill_holes)), max_cells=int(max_cells), max_fill=int(max_fill))


def is_on(r):
    return bool(r and (r["thin_above"] or r["fill_holes"]))


def new_stats():
    return dict.fromkeys(STAT_NAMES, 0)


def _limit(v):
    return v if v else DEFAULT_LIMIT


def rng_float(state):
    """randf() (main.c:203-207) off the xorshift64* stream -> (np.float32 in [0, 1], the state behind it)"""
    x = int(state)
    x ^= x >> 12
    x ^= (x << 25) & M64
    x ^= x >> 27
    hi = ((x * 0x2545F4914F6CDD1D) & M64) >> 32
    return F32(hi / 4294967295.0), x


def subcell(m, c):
    """min((int)floorf((m - (float)c) * 4.f), 3), in float32; arrays or scalars"""
    m = np.asarray(m, F32)
    return np.minimum(np.floor((m - np.asarray(c).astype(F32)) * F32(4)).astype(np.int64), 3)


def swap_with_last(m, gone):
    """refresh_marker_counts' removal (main.c:105-116) over delete flags that travel with their markers, for any number of markers: with D flags and n' = n - D the
    survivors below n' stay and the k-th hole below n' (ascending) takes the k-th survivor at or above n' counted from the back (edit_ref.delete_in_box_vectorised)"""
    n1 = len(m) - int(gone.sum())
    out = m[:n1].copy()
    out[np.nonzero(gone[:n1])[0]] = m[n1:][~gone[n1:]][::-1]
    return out


def holes_of(count, prev_count, solid, sink, source):
    """the hole mask (Y, X): interior, count == 0 and prev_count != 0, no mask of its own, all eight neighbours count != 0 or solid"""
    wet = (np.asarray(count) != 0) | (np.asarray(solid) != 0)
    Y, X = wet.shape
    around = np.ones((Y - 2, X - 2), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                around &= wet[1 + dy:Y - 1 + dy, 1 + dx:X - 1 + dx]
    hole = np.zeros((Y, X), bool)
    inner = (slice(1, Y - 1), slice(1, X - 1))
    hole[inner] = ((np.asarray(count)[inner] == 0) & (np.asarray(prev_count)[inner] != 0) & (np.asarray(solid)[inner] == 0) & (np.asarray(sink)[inner] == 0)
                   & (np.asarray(source)[inner] == 0) & around)
    return hole


def pass_arrays(r, markers, count, prev_count, solid, sink, source, rng_state, max_markers, stats=None):
    """One pass.  markers (n, 2) float32 in array order; count (Y, X) uint8 is changed in place.  -> (markers, rng_state)"""
    stats = new_stats() if stats is None else stats
    m = np.array(markers, F32).reshape(-1, 2)
    Y, X = count.shape
    flat = count.reshape(-1)
    if r["thin_above"]:
        crowded = np.nonzero(flat > r["thin_above"])[0]
        listed = crowded[:_limit(r["max_cells"])]
        stats["deferred"] += len(crowded) - len(listed)
        stats["cells_thinned"] += len(listed)
        if len(listed) and len(m):
            rank = np.full(X * Y, -1, np.int64)
            rank[listed] = np.arange(len(listed))
            cx, cy = np.floor(m[:, 0]).astype(np.int64), np.floor(m[:, 1]).astype(np.int64)
            k = rank[cy * X + cx]
            idx = np.nonzero(k >= 0)[0]      # ascending: np.unique's first occurrence of a slot is its lowest array index
            slot = 16 * k[idx] + 4 * subcell(m[idx, 1], cy[idx]) + subcell(m[idx, 0], cx[idx])
            taken, first = np.unique(slot, return_index=True)
            gone = np.zeros(len(m), bool)
            gone[idx] = True
            gone[idx[first]] = False
            stats["removed"] += int(gone.sum())
            m = swap_with_last(m, gone)
            flat[listed] = np.bincount(taken // 16, minlength=len(listed)).astype(np.uint8)
    if r["fill_holes"]:
        holes = np.nonzero(holes_of(count, prev_count, solid, sink, source).reshape(-1))[0]
        room = max(0, int(max_markers) - 1 - len(m))
        n_app = min(len(holes), _limit(r["max_fill"]), room)
        stats["deferred"] += len(holes) - n_app
        stats["added"] += n_app
        new = np.zeros((n_app, 2), F32)
        for j, c in enumerate(holes[:n_app]):
            ry, rng_state = rng_float(rng_state)      # y first, as update_fluid_sources spends its draws (main.c:288)
            rx, rng_state = rng_float(rng_state)
            new[j] = (F32(int(c) % X) + rx, F32(int(c) // X) + ry)
            flat[c] = 1
        m = np.concatenate([m, new])
    return m, int(rng_state)


def pass_loops(r, markers, count, prev_count, solid, sink, source, rng_state, max_markers, stats=None):
    """pass_arrays sentence by sentence in plain loops"""
    stats = new_stats() if stats is None else stats
    m = [(F32(x), F32(y)) for x, y in np.array(markers, F32).reshape(-1, 2)]
    Y, X = count.shape
    if r["thin_above"]:
        listed = {}
        for y in range(Y):
            for x in range(X):
                if int(count[y, x]) > r["thin_above"]:
                    if len(listed) < _limit(r["max_cells"]):
                        listed[(x, y)] = set()
                    else:
                        stats["deferred"] += 1
        gone = []
        for px, py in m:      # the flags before any deletion; ascending index: the first marker met in a sub-cell is the survivor
            cx, cy = int(np.floor(px)), int(np.floor(py))
            g = False
            if (cx, cy) in listed:
                sub = (min(int(np.floor(F32(F32(px - F32(cx)) * F32(4)))), 3), min(int(np.floor(F32(F32(py - F32(cy)) * F32(4)))), 3))
                g = sub in listed[(cx, cy)]
                listed[(cx, cy)].add(sub)
            gone.append(g)
        n, i = len(m), 0
        while i < n:      # m[i--] = m[--n]
            if gone[i]:
                n -= 1
                m[i], gone[i] = m[n], gone[n]
                stats["removed"] += 1
            else:
                i += 1
        m = m[:n]
        for (x, y), subs in listed.items():
            count[y, x] = len(subs)
        stats["cells_thinned"] += len(listed)
    if r["fill_holes"]:
        holes = []
        for y in range(1, Y - 1):
            for x in range(1, X - 1):
                if count[y, x] != 0 or prev_count[y, x] == 0 or solid[y, x] or sink[y, x] or source[y, x]:
                    continue
                if all(count[y + dy, x + dx] != 0 or solid[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                    holes.append((x, y))
        listed = 0
        for x, y in holes:
            if listed == _limit(r["max_fill"]) or len(m) + 1 > int(max_markers) - 1:
                stats["deferred"] += 1
                continue
            listed += 1
            ry, rng_state = rng_float(rng_state)
            rx, rng_state = rng_float(rng_state)
            m.append((F32(F32(x) + rx), F32(F32(y) + ry)))
            count[y, x] = 1
            stats["added"] += 1
    return np.array(m, F32).reshape(-1, 2), int(rng_state)


def pass_c(r, markers, count, prev_count, solid, sink, source, rng_state, max_markers, stats=None):
    """the library's own sequential reference (euler_host.c eu_reseed_pass; host code, no GPU)"""
    stats = new_stats() if stats is None else stats
    L = ea.load_library()
    L.eu_reseed_pass.restype = C.c_int
    L.eu_reseed_pass.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    rec = ea.reseed(r["thin_above"], r["fill_holes"], r["max_cells"], r["max_fill"])
    rec = np.ascontiguousarray(rec).reshape(1)
    Y, X = count.shape
    src = np.array(markers, F32).reshape(-1, 2)
    buf = np.zeros((max(int(max_markers), len(src)) + 1, 2), F32)
    buf[:len(src)] = src
    n, rng, st = C.c_uint64(len(src)), C.c_uint64(int(rng_state)), np.zeros((), ea.RESEED_STATS_DTYPE)
    grids = [np.ascontiguousarray(g, np.uint8) for g in (prev_count, solid, sink, source)]
    assert count.flags.c_contiguous and count.dtype == np.uint8
    rc = L.eu_reseed_pass(rec.ctypes.data, X, Y, buf.ctypes.data, C.addressof(n), int(max_markers), count.ctypes.data, *[g.ctypes.data for g in grids],
                          C.addressof(rng), st.ctypes.data)
    assert rc == 0, rc
    for k in STAT_NAMES:
        stats[k] += int(st[k])
    return buf[:n.value].copy(), int(rng.value)


def apply(o, r, stats=None, fn=pass_arrays):
    """the pass on an oracle's arrays, where it stands: right behind eo_refresh_marker_counts"""
    if not is_on(r):
        return
    m, rng = fn(r, o.markers, o.count, o.prev_count, o.solid, o.sink, o.source, int(o.c.rng_state), 4 * o.X * o.Y, stats)
    o.set_markers(m)
    o.c.rng_state = rng


def substep(am, o, dt, r, stats=None, clock=None, f=None, boxes=(), rk2=False, mc=False, acc_at=None, heat=None):
    """forcing_ref.substep (eo_substep, main.c:855-898) with the pass behind the refresh: in front of the dye's and the temperature's extension, the sources and
    extrapolate, which all see the counts it leaves.  heat = (T, record, boxes) as bodies_ref.substep takes it.  Returns the PCG iterations."""
    lib = o.lib
    clock = fref.Clock() if clock is None else clock
    if rk2:
        am.ar_advect_markers(C.cast(o.ptr, C.c_void_p), C.c_float(dt), 1)
    else:
        lib.eo_advect_markers(o.ptr, C.c_float(dt))
    lib.eo_refresh_marker_counts(o.ptr)
    apply(o, r, stats)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            lib.eo_extrapolate(o.ptr, o.f32p(q), fref.P)
    lib.eo_update_fluid_sources(o.ptr)
    if heat is not None:
        href.extend(o, heat[0], heat[1])
    lib.eo_extrapolate(o.ptr, o.f32p(o.u), fref.U)
    lib.eo_extrapolate(o.ptr, o.f32p(o.v), fref.V)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.u), fref.U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.v), fref.V)
    acc = None if (acc_at is None or f is None) else acc_at(f, clock.t)
    if heat is not None:
        href.advect_velocity_stage(am, o, heat[0], heat[1], heat[2], dt, f, boxes, clock.t, rk2, mc, acc)
    else:
        fref.advect_velocity_stage(am, o, dt, fref.DEFAULT if f is None else f, boxes, clock.t, rk2, mc, acc)
    it = lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    o.c.total_substeps += 1
    o.c.last_dt = dt
    clock.advance(dt)
    return it


def step(am, o, r, stats=None, clock=None, f=None, boxes=(), rk2=False, mc=False, acc_at=None, heat=None, frame_time=0.1, max_substeps=8):
    """eo_step (main.c:843-853) over substep above -> (substeps, PCG iterations)"""
    clock = fref.Clock() if clock is None else clock
    ft = F32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = F32(ft - dt)
        iters += substep(am, o, float(dt), r, stats, clock, f, boxes, rk2, mc, acc_at, heat)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return n, iters
