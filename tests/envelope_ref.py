"""Test-side restatement of the run-long envelopes (euler_set_envelope, include/euler.h, docs/envelope.md): arrival time, wet time, peak speed squared and
peak pressure per cell, the raster over them and its image.

Written from the header's rules, not from the kernels: the yardstick of test_envelope_host.py and test_gpu_envelope.py.
  Envelope           the planes of the enabled channels as numpy arrays (uint32 words; .f(channel) views them as float32)
  update / update_loop   the update at the end of one substep, in numpy float32 operations and cell by cell in plain loops
  raster / raster_loop   euler_envelope_raster: the pixel boxes of euler_overview_box, integer sums and extremes of bit patterns
  rgb / rgb_loop     euler_envelope_rgb in Python doubles
  fold               update() on a handle's or an oracle's arrays as they stand
  substep / step     compose a substep over forcing_ref's composition of the oracle's exported stage functions (RK1 / RK2 / MacCormack, any forcing), with its
                     double clock: t_end = (float)(t + (double)dt) is formed from the clock BEFORE the substep
Test infrastructure only: nothing under euler_amd/ imports this module."""
import math

import numpy as np

import forcing_ref as fref

ARRIVAL, WET, SPEED, PRESSURE, ALL = 1, 2, 4, 8, 15
CHANNELS = (ARRIVAL, WET, SPEED, PRESSURE)
NAMES = {ARRIVAL: "arrival", WET: "wet", SPEED: "speed", PRESSURE: "pressure"}
NEVER = np.uint32(0xFFFFFFFF)
F32 = np.float32
PX_DTYPE = np.dtype({"names": ["cells", "touched", "arrival_min", "arrival_max", "wet_max", "speed2_max", "p_max", "reserved"],
                     "formats": [np.uint32] * 8, "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})
PX_FIELD = {ARRIVAL: "arrival_min", WET: "wet_max", SPEED: "speed2_max", PRESSURE: "p_max"}


class Envelope:
    """planes[channel]: uint32 (Y, X), only for the enabled channels; substeps as euler_get_envelope counts them"""

    def __init__(self, X, Y, channels=ALL):
        self.X, self.Y, self.channels, self.substeps = X, Y, channels, 0
        self.planes = {c: np.full((Y, X), NEVER if c == ARRIVAL else 0, np.uint32) for c in CHANNELS if channels & c}

    def f(self, channel):
        return self.planes[channel].view(F32)

    def copy(self):
        e = Envelope(self.X, self.Y, 0)
        e.channels, e.substeps = self.channels, self.substeps
        e.planes = {c: p.copy() for c, p in self.planes.items()}
        return e


def fluid_cells(solid, count):
    """interior cells with count != 0 && !solid, as the gauges define a fluid cell"""
    f = (np.asarray(count) != 0) & (np.asarray(solid) == 0)
    f[0, :] = f[-1, :] = False
    f[:, 0] = f[:, -1] = False
    return f


def t_end_of(t, dt):
    return F32(np.float64(t) + np.float64(F32(dt)))


def speed2(u, v):
    """ObRow::speed2 on every cell that has a left and a lower neighbour (row 0 and column 0: 0), float32 operation by operation"""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    s2 = np.zeros(u.shape, F32)
    with np.errstate(all="ignore"):
        dx = (u[1:, 1:] + u[1:, :-1]) / F32(2)
        dy = (v[1:, 1:] + v[:-1, 1:]) / F32(2)
        s2[1:, 1:] = dx * dx + dy * dy
    return s2


def _max_bits(plane, where, x):
    """ob_max_bits on the cells `where`: a NaN is skipped, else the larger bit pattern stays"""
    bits = np.ascontiguousarray(x, F32).view(np.uint32)
    take = where & ~np.isnan(x) & (bits > plane)
    plane[take] = bits[take]


def update(env, solid, count, u, v, p, t, dt):
    """One substep's update from the state EULER_STAGE_PROJECT leaves; t is the clock before the substep."""
    fl = fluid_cells(solid, count)
    dt = F32(dt)
    if env.channels & ARRIVAL:
        a = env.planes[ARRIVAL]
        a[fl & (a == NEVER)] = np.array(t_end_of(t, dt), F32).view(np.uint32)
    if env.channels & WET:
        w = env.f(WET)
        w[fl] = w[fl] + dt
    if env.channels & SPEED:
        _max_bits(env.planes[SPEED], fl, speed2(u, v))
    if env.channels & PRESSURE:
        with np.errstate(all="ignore"):
            pf = np.asarray(p, np.float64).astype(F32)
        _max_bits(env.planes[PRESSURE], fl, np.where(pf > 0, pf, F32(0)).astype(F32))
    env.substeps += 1


def update_loop(env, solid, count, u, v, p, t, dt):
    """update() cell by cell in plain loops, scalar np.float32 arithmetic"""
    Y, X = np.asarray(count).shape
    dt = F32(dt)
    te = int(np.array(t_end_of(t, dt), F32).view(np.uint32))

    def bits(x):
        return int(np.array(x, F32).view(np.uint32))

    with np.errstate(all="ignore"):
        for y in range(1, Y - 1):
            for x in range(1, X - 1):
                if not count[y, x] or solid[y, x]:
                    continue
                if env.channels & ARRIVAL and int(env.planes[ARRIVAL][y, x]) == 0xFFFFFFFF:
                    env.planes[ARRIVAL][y, x] = te
                if env.channels & WET:
                    env.f(WET)[y, x] = F32(env.f(WET)[y, x] + dt)
                if env.channels & SPEED:
                    dx = F32(F32(F32(u[y, x]) + F32(u[y, x - 1])) / F32(2))
                    dy = F32(F32(F32(v[y, x]) + F32(v[y - 1, x])) / F32(2))
                    s2 = F32(F32(dx * dx) + F32(dy * dy))
                    if s2 == s2 and bits(s2) > int(env.planes[SPEED][y, x]):
                        env.planes[SPEED][y, x] = bits(s2)
                if env.channels & PRESSURE:
                    pf = F32(p[y, x])
                    val = pf if pf > 0 else F32(0)
                    if bits(val) > int(env.planes[PRESSURE][y, x]):
                        env.planes[PRESSURE][y, x] = bits(val)
    env.substeps += 1


# ----------------------------------------------------------------------------- the raster
def pixel_edges(lo, n, W):
    """the first cell of every pixel column of a box of n cells from `lo` on, and one behind the last: x0 + floor(px * Bw / W)"""
    return [lo + (k * n) // W for k in range(W + 1)]


def pixel_rows(y0, y1, H):
    """(ytop, ybot) per pixel row, row 0 = the top: y1 - floor(py * Bh / H) down to y1 + 1 - floor((py + 1) * Bh / H)"""
    Bh = y1 - y0 + 1
    return [(y1 - (py * Bh) // H, y1 + 1 - ((py + 1) * Bh) // H) for py in range(H)]


def raster(env, box, W, H):
    x0, y0, x1, y1 = box
    xs = pixel_edges(x0, x1 - x0 + 1, W)
    out = np.zeros((H, W), PX_DTYPE)
    out["arrival_min"] = NEVER
    for py, (ytop, ybot) in enumerate(pixel_rows(y0, y1, H)):
        for px in range(W):
            b = (slice(ybot, ytop + 1), slice(xs[px], xs[px + 1]))
            r = out[py, px]
            r["cells"] = (ytop - ybot + 1) * (xs[px + 1] - xs[px])
            if env.channels & ARRIVAL:
                a = env.planes[ARRIVAL][b]
                hit = a != NEVER
                r["touched"] = hit.sum()
                r["arrival_min"] = a.min()
                r["arrival_max"] = a[hit].max() if hit.any() else 0
            for c in (WET, SPEED, PRESSURE):
                if env.channels & c:
                    r[PX_FIELD[c]] = env.planes[c][b].max()
    return out


def raster_loop(env, box, W, H):
    """raster() from the cell's side: every cell of the box finds its pixel, py(y) = ((y1 - y + 1) H - 1) / Bh and px(x) = ((x - x0 + 1) W - 1) / Bw"""
    x0, y0, x1, y1 = box
    Bw, Bh = x1 - x0 + 1, y1 - y0 + 1
    out = np.zeros((H, W), PX_DTYPE)
    out["arrival_min"] = NEVER
    for y in range(y0, y1 + 1):
        py = ((y1 - y + 1) * H - 1) // Bh
        for x in range(x0, x1 + 1):
            r = out[py, ((x - x0 + 1) * W - 1) // Bw]
            r["cells"] += 1
            if env.channels & ARRIVAL:
                a = env.planes[ARRIVAL][y, x]
                r["arrival_min"] = min(r["arrival_min"], a)
                if a != NEVER:
                    r["touched"] += 1
                    r["arrival_max"] = max(r["arrival_max"], a)
            for c in (WET, SPEED, PRESSURE):
                if env.channels & c:
                    r[PX_FIELD[c]] = max(r[PX_FIELD[c]], env.planes[c][y, x])
    return out


def _value(rec, channel):
    return float(np.array(rec[PX_FIELD[channel]], np.uint32).view(F32))


def rgb_loop(px, channel, scale):
    H, W = px.shape
    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            r = px[y, x]
            dark = r["touched"] == 0 if channel == ARRIVAL else (r["touched"] == 0 and r[PX_FIELD[channel]] == 0)
            if dark:
                continue
            val = _value(r, channel)
            if channel == SPEED:
                val = math.sqrt(val) if val == val and val >= 0 else float("nan")
            t = val / scale
            t = (t if t < 1.0 else 1.0) if t > 0.0 else 0.0
            c = int(255.0 * (1.0 - t))
            out[y, x] = (255, c, c)
    return out


def rgb(px, channel, scale):
    words = np.ascontiguousarray(px[PX_FIELD[channel]])
    with np.errstate(all="ignore"):
        val = words.view(F32).astype(np.float64)
        if channel == SPEED:
            val = np.sqrt(val)
        t = val / np.float64(scale)
        t = np.where(t > 0.0, np.where(t < 1.0, t, 1.0), 0.0)
        c = (255.0 * (1.0 - t)).astype(np.int64).astype(np.uint8)
    dark = (px["touched"] == 0) if channel == ARRIVAL else ((px["touched"] == 0) & (words == 0))
    out = np.stack([np.full(px.shape, 255, np.uint8), c, c], axis=-1)
    out[dark] = 0
    return out


# ----------------------------------------------------------------------------- on a handle's read-backs and on the oracle
def fold(env, src, t, dt, get=None):
    """update() from an oracle (get = None: its arrays) or from a handle's read-backs (get(field_name) -> array)"""
    names = ("solid", "count", "u", "v", "p")
    g = [np.array(getattr(src, n)) for n in names] if get is None else [get(n) for n in names]
    update(env, *g, t, dt)


def front_half(am, o, dt, t, f=None, boxes=(), rk2=False, mc=False, acc_at=None):
    """the five stages in front of EULER_STAGE_PROJECT, as forcing_ref.substep composes them over the oracle's exported functions"""
    import ctypes as C
    from oracle_lib import P, U, V
    lib, f = o.lib, f or fref.DEFAULT
    if rk2:
        am.ar_advect_markers(C.cast(o.ptr, C.c_void_p), C.c_float(dt), 1)
    else:
        lib.eo_advect_markers(o.ptr, C.c_float(dt))
    lib.eo_refresh_marker_counts(o.ptr)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            lib.eo_extrapolate(o.ptr, o.f32p(q), P)
    lib.eo_update_fluid_sources(o.ptr)
    lib.eo_extrapolate(o.ptr, o.f32p(o.u), U)
    lib.eo_extrapolate(o.ptr, o.f32p(o.v), V)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.u), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.v), V)
    fref.advect_velocity_stage(am, o, dt, f, list(boxes), t, rk2, mc, None if acc_at is None else acc_at(f, t))


def project(o, env, dt, t):
    """EULER_STAGE_PROJECT with the hook at its end: eo_project, then the update from what it leaves, with the clock t of the substep's start"""
    import ctypes as C
    it = o.lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    fold(env, o, t, dt)
    return it


def substep(am, o, env, dt, clock, f=None, boxes=(), rk2=False, mc=False, acc_at=None):
    """a substep stage by stage (with RK1 and the default forcing: eo_substep); the clock advances behind it"""
    front_half(am, o, dt, clock.t, f, boxes, rk2, mc, acc_at)
    it = project(o, env, dt, clock.t)
    o.c.total_substeps += 1
    o.c.last_dt = dt
    clock.advance(dt)
    return it


def step(am, o, env, clock, f=None, boxes=(), rk2=False, mc=False, acc_at=None, frame_time=0.1, max_substeps=8, on_substep=None):
    """forcing_ref.step with the update behind every substep; on_substep(k, n_left) is called behind each (the preconditions' probe)"""
    import ctypes as C
    ft = F32(frame_time)
    n = 0
    while ft > 0 and n < max_substeps:
        dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = F32(ft - dt)
        substep(am, o, env, float(dt), clock, f, boxes, rk2, mc, acc_at)
        n += 1
        if on_substep:
            on_substep(n, bool(ft > 0 and n < max_substeps))
    o.c.last_substeps = n
    o.c.frame_count += 1
    return n
