"""Test-side restatement of the temperature (euler_set_heat, include/euler.h, docs/heat.md): an advected scalar with buoyancy, heaters and diffusion.

Written from the header's rules, not from the kernels: the yardstick of test_heat_host.py and test_gpu_heat.py.
  extend           STAGE_SOURCES: the oracle's eo_extrapolate(T, P) with the cells that had no fluid neighbour at ambient, then the source cells
  transport        step a: the oracle's eo_advect_p, tests/c/advect_rk2.c's ar_advect_p or advect_maccormack_ref.advect_p; only fluid cells take the result
  after_transport_arrays   steps b - e in np.float32 array operations: boxes in list order, Jacobi diffusion, ambient in the dry cells, buoyancy on utmp / vtmp
  after_transport_loop     the same in plain Python loops (a second restatement)
  raster / paint   euler_heat_raster and euler_heat_paint in numpy: integer sums, bit-pattern maxima, the painter's doubles
  advect_velocity_stage / substep / step   compose a substep as forcing_ref does, with forcing_ref.apply for the uniform part and the force boxes and the
                   heat between that and eo_zero_bounds

A heat record is a dict with the keys of DEFAULT (missing ones take the defaults); boxes is a list of (kind, value, (x0, y0, x1, y1)), kind FIX or RATE.
T is a C-contiguous np.float32 array of shape (Y, X) that the functions change in place.
Test infrastructure only: nothing under euler_amd/ imports this module."""
import ctypes as C

import numpy as np

import advect_maccormack_ref as amref
import forcing_ref as fref
from oracle_lib import P, U, V

FIX, RATE = 0, 1
DEFAULT = dict(ambient=0.0, beta=0.0, kappa=0.0, source_t=0.0)
F32 = np.float32


def heat(ambient=0.0, beta=0.0, kappa=0.0, source_t=0.0):
    return dict(ambient=float(ambient), beta=float(beta), kappa=float(kappa), source_t=float(source_t))


def field(o, h):
    """the field behind switching on: ambient everywhere"""
    return np.full((o.Y, o.X), F32(dict(DEFAULT, **h)["ambient"]), F32)


# ----------------------------------------------------------------------------- STAGE_SOURCES
def extend(o, T, h):
    """behind eo_refresh_marker_counts (the source update changes counts in source cells only, and those take source_t): a cell that just became fluid takes
    the mean of its previously-fluid 3 x 3 neighbours - the oracle's sum and division -, ambient where it has none; then every source cell takes source_t"""
    h = dict(DEFAULT, **h)
    prev, cur = np.asarray(o.prev_count) != 0, np.asarray(o.count) != 0
    pad = np.zeros((o.Y + 2, o.X + 2), np.int32)
    pad[1:-1, 1:-1] = prev
    n = sum(pad[1 + dy:o.Y + 1 + dy, 1 + dx:o.X + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    lonely = ~prev & cur & (n == 0)
    with np.errstate(all="ignore"):
        o.lib.eo_extrapolate(o.ptr, o.f32p(T), P)
    T[lonely] = F32(h["ambient"])
    T[np.asarray(o.source) != 0] = F32(h["source_t"])
    return int(lonely.sum())


# ----------------------------------------------------------------------------- STAGE_ADVECT_VELOCITY
def transport(am, o, T, dt, rk2=False, mc=False):
    """step a: T as one dye channel under the transport options, from the stage's input o.u, o.v; only fluid cells take the result"""
    tmp = T.copy()
    if mc:
        res = T.copy()
        amref.advect_p(am, o, res, o.u, o.v, dt, tmp, rk2, mc)      # (the corrected channel comes back in its first array)
    elif rk2:
        am.ar_advect_p(C.cast(o.ptr, C.c_void_p), o.f32p(T), o.f32p(o.u), o.f32p(o.v), C.c_float(dt), o.f32p(tmp), 1)
        res = tmp
    else:
        o.lib.eo_advect_p(o.ptr, o.f32p(T), o.f32p(o.u), o.f32p(o.v), C.c_float(dt), o.f32p(tmp))
        res = tmp
    cn = np.asarray(o.count) != 0
    T[cn] = res[cn]


def after_transport_arrays(T, utmp, vtmp, solid, count, h, boxes, dt, acc):
    """steps b - e in place, every operation a float32 operation of numpy"""
    h = dict(DEFAULT, **h)
    amb, beta, kappa, dt = F32(h["ambient"]), F32(h["beta"]), F32(h["kappa"]), F32(dt)
    ax, ay = F32(acc[0]), F32(acc[1])
    cn = np.asarray(count) != 0
    for kind, value, (x0, y0, x1, y1) in boxes:      # b
        b = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        sub, m = T[b], cn[b]      # a view
        if kind == FIX:
            sub[m] = F32(value)
        else:
            sub[m] = sub[m] + F32(F32(value) * dt)
    if kappa > 0:      # c
        c = F32(kappa * dt)
        acc_ = np.zeros(T.shape, F32)
        for axis, shift in ((1, 1), (1, -1), (0, 1), (0, -1)):      # left, right, lower, upper (a fluid cell never lies on the border ring: no wrap reaches one)
            Tn, fn = np.roll(T, shift, axis), np.roll(cn, shift, axis)
            acc_ = np.where(fn, acc_ + (Tn - T), acc_).astype(F32)
        T[cn] = (T + c * acc_)[cn]
    T[~cn] = amb      # d
    if beta != 0:      # e
        lu, lv = fref.live_faces(solid, count)
        ga = F32(ay * dt)
        a, b = T[:-1, :], T[1:, :]
        ca, cb = cn[:-1, :], cn[1:, :]
        tf = np.where(ca & cb, (a + b) / F32(2), np.where(ca, a, b)).astype(F32)
        d = tf - amb
        m = lv[:-1, :] & (d != 0)
        sv = vtmp[:-1, :]
        sv[m] = sv[m] - (beta * d[m]) * ga
        if ax != 0:
            ga = F32(ax * dt)
            a, b = T[:, :-1], T[:, 1:]
            ca, cb = cn[:, :-1], cn[:, 1:]
            tf = np.where(ca & cb, (a + b) / F32(2), np.where(ca, a, b)).astype(F32)
            d = tf - amb
            m = lu[:, :-1] & (d != 0)
            su = utmp[:, :-1]
            su[m] = su[m] - (beta * d[m]) * ga


def after_transport_loop(T, utmp, vtmp, solid, count, h, boxes, dt, acc):
    """after_transport_arrays cell by cell and face by face in plain loops, scalar np.float32 arithmetic"""
    h = dict(DEFAULT, **h)
    Y, X = count.shape
    amb, beta, kappa, dt = F32(h["ambient"]), F32(h["beta"]), F32(h["kappa"]), F32(dt)
    ax, ay = F32(acc[0]), F32(acc[1])
    for kind, value, (x0, y0, x1, y1) in boxes:
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                if count[y, x]:
                    T[y, x] = F32(value) if kind == FIX else F32(T[y, x] + F32(F32(value) * dt))
    if kappa > 0:
        c = F32(kappa * dt)
        old = T.copy()
        for y in range(Y):
            for x in range(X):
                if not count[y, x]:
                    continue
                a = F32(0)
                for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if count[yy, xx]:
                        a = F32(a + F32(old[yy, xx] - old[y, x]))
                T[y, x] = F32(old[y, x] + F32(c * a))
    for y in range(Y):
        for x in range(X):
            if not count[y, x]:
                T[y, x] = amb
    if beta == 0:
        return

    def face(y, x, y2, x2, q, g):
        if not (count[y, x] or count[y2, x2]) or solid[y, x] or solid[y2, x2]:
            return
        if count[y, x] and count[y2, x2]:
            tf = F32(F32(T[y, x] + T[y2, x2]) / F32(2))
        else:
            tf = T[y, x] if count[y, x] else T[y2, x2]
        d = F32(tf - amb)
        if d != 0:
            q[y, x] = F32(q[y, x] - F32(F32(beta * d) * g))

    for y in range(Y):
        for x in range(X):
            if y < Y - 1:
                face(y, x, y + 1, x, vtmp, F32(ay * dt))
            if x < X - 1 and ax != 0:
                face(y, x, y, x + 1, utmp, F32(ax * dt))


def acc_of(f, t, acc=None):
    """the substep's uniform acceleration: (0, -10) without a forcing"""
    if acc is not None:
        return acc
    return (F32(0), F32(-10)) if f is None else fref.forcing_at(f, t)


def advect_velocity_stage(am, o, T, h, hboxes, dt, f=None, fboxes=(), t=0.0, rk2=False, mc=False, acc=None, after=after_transport_arrays):
    """What the product's STAGE_ADVECT_VELOCITY leaves in utmp / vtmp, the dye and T: forcing_ref.advect_velocity_stage with the heat between the force boxes
    and zero_bounds.  f = None: the reference's gravity."""
    lib = o.lib
    dtc = C.c_float(dt)
    a = acc_of(f, t, acc)
    if mc:
        if o.c.rainbow:
            for q, tmp in ((o.cr, o.crtmp), (o.cg, o.cgtmp), (o.cb, o.cbtmp)):
                amref.advect_p(am, o, q, o.u, o.v, dt, tmp, rk2, mc)
        amref.advect_u(am, o, o.u, o.v, dt, o.utmp, rk2, mc)
        amref.advect_v(am, o, o.u, o.v, dt, o.vtmp, rk2, mc)
    elif rk2:
        p = C.cast(o.ptr, C.c_void_p)
        am.ar_advect_u(p, o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(o.utmp), 1)
        am.ar_advect_v(p, o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(o.vtmp), 1)
        if o.c.rainbow:
            for q, tmp in ((o.cr, o.crtmp), (o.cg, o.cgtmp), (o.cb, o.cbtmp)):
                am.ar_advect_p(p, o.f32p(q), o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(tmp), 1)
                q[...] = tmp
    else:
        lib.eo_advect_u(o.ptr, o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(o.utmp))
        lib.eo_advect_v(o.ptr, o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(o.vtmp))
        if o.c.rainbow:
            for q, tmp in ((o.cr, o.crtmp), (o.cg, o.cgtmp), (o.cb, o.cbtmp)):
                lib.eo_advect_p(o.ptr, o.f32p(q), o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(tmp))
                q[...] = tmp
    fref.apply(o, f or fref.DEFAULT, list(fboxes), t, dt, a)
    transport(am, o, T, dt, rk2, mc)
    after(T, o.utmp, o.vtmp, np.asarray(o.solid), np.asarray(o.count), h, hboxes, dt, a)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.utmp), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.vtmp), V)
    if o.c.viscosity > 0.0:
        fref._bind_diffuse(lib)
        lib.eo_diffuse(o.ptr, o.f32p(o.utmp), U, dtc, o.f32p(o.u))
        lib.eo_diffuse(o.ptr, o.f32p(o.vtmp), V, dtc, o.f32p(o.v))
        o.utmp[:, :-1] = o.u[:, :-1]
        o.vtmp[:-1, :] = o.v[:-1, :]


def substep(am, o, T, h, hboxes, dt, f=None, fboxes=(), clock=None, rk2=False, mc=False, acc_at=None):
    """eo_substep with the heat in its two stages; the forcing is taken at the clock's time at the start, the clock advances behind it.  Returns the PCG iterations."""
    lib = o.lib
    clock = clock or fref.Clock()
    if rk2:
        am.ar_advect_markers(C.cast(o.ptr, C.c_void_p), C.c_float(dt), 1)
    else:
        lib.eo_advect_markers(o.ptr, C.c_float(dt))
    lib.eo_refresh_marker_counts(o.ptr)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            lib.eo_extrapolate(o.ptr, o.f32p(q), P)
    lib.eo_update_fluid_sources(o.ptr)
    extend(o, T, h)
    lib.eo_extrapolate(o.ptr, o.f32p(o.u), U)
    lib.eo_extrapolate(o.ptr, o.f32p(o.v), V)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.u), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.v), V)
    acc = None if (acc_at is None or f is None) else acc_at(f, clock.t)
    advect_velocity_stage(am, o, T, h, hboxes, dt, f, fboxes, clock.t, rk2, mc, acc)
    it = lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    o.c.total_substeps += 1
    o.c.last_dt = dt
    clock.advance(dt)
    return it


def step(am, o, T, h, hboxes, f=None, fboxes=(), clock=None, rk2=False, mc=False, acc_at=None, frame_time=0.1, max_substeps=8):
    """eo_step: CFL substeps until the frame time is used up, at most 8"""
    clock = clock or fref.Clock()
    ft = F32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = F32(ft - dt)
        iters += substep(am, o, T, h, hboxes, float(dt), f, fboxes, clock, rk2, mc, acc_at)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return n, iters


# ----------------------------------------------------------------------------- the raster and its painter
PX_DTYPE = np.dtype({"names": ["cells", "water", "t_pos", "t_neg", "max_above", "max_below"], "formats": [np.uint32] * 2 + [np.uint64] * 2 + [np.float32] * 2,
                     "offsets": [0, 4, 8, 16, 24, 28], "itemsize": 32})


def qv(a):
    """min(a, 4096) * 2^20, truncated, for a >= 0 (an infinity: the clamp); exact in float32: a power of two times a float below 2^12"""
    return int(F32(min(F32(a), F32(4096))) * F32(1048576))


def raster(T, solid, sink, count, ambient, box, W, H):
    """euler_heat_raster cell by cell: the pixel of a cell by euler_overview_box's edges (pixel px holds the columns x0 + floor(px Bw / W) ... , rows from the
    top), water = no solid, no sink, markers; d = fl(T - ambient) to the sum of its sign and the maximum of its side; a NaN to neither"""
    x0, y0, x1, y1 = box
    Bw, Bh = x1 - x0 + 1, y1 - y0 + 1
    out = np.zeros((H, W), PX_DTYPE)
    for py in range(H):
        for px in range(W):
            out[py, px]["cells"] = (((px + 1) * Bw) // W - (px * Bw) // W) * (((py + 1) * Bh) // H - (py * Bh) // H)
    for y in range(y0, y1 + 1):
        py = ((y1 - y + 1) * H - 1) // Bh
        for x in range(x0, x1 + 1):
            if solid[y, x] or sink[y, x] or not count[y, x]:
                continue
            r = out[py, ((x - x0 + 1) * W - 1) // Bw]
            r["water"] += 1
            with np.errstate(all="ignore"):
                d = F32(T[y, x]) - F32(ambient)
            if d != d:
                continue
            side, mx = ("t_pos", "max_above") if d >= 0 else ("t_neg", "max_below")
            a = abs(d)
            r[side] += np.uint64(qv(a))
            if a > 0 and F32(a).view(np.uint32) > r[mx].view(np.uint32):
                r[mx] = a
    return out


def paint(heat, scale):
    """euler_heat_paint -> the three dye sums per pixel, uint64 of shape (h, w, 3): m = (t_pos - t_neg) / 2^20 / water in doubles, t = clamp(m / scale, -1, 1),
    white to red above, white to blue below, water * q24(colour)"""
    h, w = heat.shape
    out = np.zeros((h, w, 3), np.uint64)
    for y in range(h):
        for x in range(w):
            f = heat[y, x]
            water = int(f["water"])
            m = (float(int(f["t_pos"])) - float(int(f["t_neg"]))) / 1048576.0 / water if water else 0.0
            t = min(max(m / scale, -1.0), 1.0)
            lin = (1.0, 1.0 - t, 1.0 - t) if t >= 0 else (1.0 + t, 1.0 + t, 1.0)
            for c in range(3):
                v = F32(lin[c])
                v = F32(0) if not v > 0 else (F32(1) if v > 1 else v)
                out[y, x, c] = water * int(v * F32(16777216))
    return out
