"""Test-side restatement of the forcing (euler_set_forcing, include/euler.h, docs/forcing.md): gravity vector, shaken tank, force boxes.

Written from the header's rules, not from the kernels: the yardstick of test_forcing_host.py and test_gpu_forcing.py.
  forcing_at       the uniform acceleration at time t, in numpy doubles
  apply_arrays     the forcing on utmp / vtmp in np.float32 operations: the `ax != 0` test, products rounded before the adds, boxes in list order
  apply_loop       the same in plain Python loops over the faces (a second restatement)
  apply            apply_arrays on an oracle's arrays: it stands where eo_apply_body_forces stands in the substep
  advect_velocity_stage / substep / step   compose a substep as advect_rk2_ref / advect_maccormack_ref do, over the oracle's exported stage
                   functions and the ar_* / am_* transports, with the restated forcing and a double clock of their own (Clock)

A forcing is a dict with the keys of FIELDS (missing ones take the defaults); boxes is a list of ((x0, y0, x1, y1), (fx, fy)).
Test infrastructure only: nothing under euler_amd/ imports this module."""
import ctypes as C

import numpy as np

import advect_maccormack_ref as amref
from oracle_lib import P, U, V

FIELDS = ("gx", "gy", "shake_x", "shake_y", "shake_hz", "shake_phase")
DEFAULT = dict(gx=0.0, gy=-10.0, shake_x=0.0, shake_y=0.0, shake_hz=0.0, shake_phase=0.0)
F32 = np.float32


def forcing(gravity=(0.0, -10.0), shake=None):
    f = dict(DEFAULT, gx=float(gravity[0]), gy=float(gravity[1]))
    if shake is not None:
        f.update(shake_x=float(shake[0]), shake_y=float(shake[1]), shake_hz=float(shake[2]), shake_phase=float(shake[3]) if len(shake) > 3 else 0.0)
    return f


def forcing_at(f, t):
    """(ax, ay) as np.float32: in double, g + shake * sin(2 pi hz t + phase), then narrowed; g and shake are float32 values"""
    f = dict(DEFAULT, **f)
    s = np.sin(np.float64(2.0 * np.pi) * np.float64(f["shake_hz"]) * np.float64(t) + np.float64(f["shake_phase"]))
    ax = np.float64(F32(f["gx"])) + np.float64(F32(f["shake_x"])) * s
    ay = np.float64(F32(f["gy"])) + np.float64(F32(f["shake_y"])) * s
    return F32(ax), F32(ay)


def live_faces(solid, count):
    """(live_u, live_v), (Y, X) bools: a face is live as the velocity advection tests it; column X - 1 of u and row Y - 1 of v do not exist"""
    cn, so = np.asarray(count) > 0, np.asarray(solid) != 0
    lu, lv = np.zeros(cn.shape, bool), np.zeros(cn.shape, bool)
    lu[:, :-1] = (cn[:, :-1] | cn[:, 1:]) & ~(so[:, :-1] | so[:, 1:])
    lv[:-1, :] = (cn[:-1, :] | cn[1:, :]) & ~(so[:-1, :] | so[1:, :])
    return lu, lv


def apply_arrays(utmp, vtmp, solid, count, acc, boxes, dt):
    """In place, float32: every live v face += fl(ay dt); every live u face += fl(ax dt) only when ax != 0; then box by box in list order, per cell of the
    box, its right face += fl(fx dt) and its top face += fl(fy dt) where live.  Faces that are not live are not touched."""
    assert utmp.dtype == F32 and vtmp.dtype == F32
    ax, ay, dt = F32(acc[0]), F32(acc[1]), F32(dt)
    lu, lv = live_faces(solid, count)
    vtmp[lv] = vtmp[lv] + F32(ay * dt)
    if ax != F32(0):
        utmp[lu] = utmp[lu] + F32(ax * dt)
    for (x0, y0, x1, y1), (fx, fy) in boxes:
        b = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        su, sv = utmp[b], vtmp[b]      # views
        su[lu[b]] = su[lu[b]] + F32(F32(fx) * dt)
        sv[lv[b]] = sv[lv[b]] + F32(F32(fy) * dt)


def apply_loop(utmp, vtmp, solid, count, acc, boxes, dt):
    """apply_arrays face by face in plain loops, scalar np.float32 arithmetic"""
    Y, X = count.shape
    ax, ay, dt = F32(acc[0]), F32(acc[1]), F32(dt)

    def live_u(y, x):
        return x < X - 1 and bool(count[y, x] or count[y, x + 1]) and not (solid[y, x] or solid[y, x + 1])

    def live_v(y, x):
        return y < Y - 1 and bool(count[y, x] or count[y + 1, x]) and not (solid[y, x] or solid[y + 1, x])

    for y in range(Y):
        for x in range(X):
            if live_v(y, x):
                vtmp[y, x] = F32(vtmp[y, x] + F32(ay * dt))
            if live_u(y, x) and ax != 0:
                utmp[y, x] = F32(utmp[y, x] + F32(ax * dt))
    for (x0, y0, x1, y1), (fx, fy) in boxes:
        pu, pv = F32(F32(fx) * dt), F32(F32(fy) * dt)
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                if live_u(y, x):
                    utmp[y, x] = F32(utmp[y, x] + pu)
                if live_v(y, x):
                    vtmp[y, x] = F32(vtmp[y, x] + pv)


def apply(o, f, boxes, t, dt, acc=None):
    """The forcing on the oracle's utmp / vtmp, where eo_apply_body_forces stands; acc = (ax, ay) overrides forcing_at(f, t) (the GPU tests take
    euler_forcing_at's own, so that no libm difference reaches them)."""
    apply_arrays(o.utmp, o.vtmp, o.solid, o.count, forcing_at(f, t) if acc is None else acc, boxes, dt)


class Clock:
    """the composition's own double clock: t += (double)dt behind every substep"""

    def __init__(self, t=0.0):
        self.t = float(t)

    def advance(self, dt):
        self.t = float(np.float64(self.t) + np.float64(F32(dt)))


def _bind_diffuse(lib):
    fp = C.POINTER(C.c_float)
    lib.eo_diffuse.argtypes = [lib.eo_create.restype, fp, C.c_int, C.c_float, fp]
    lib.eo_diffuse.restype = None


def advect_velocity_stage(am, o, dt, f, boxes, t, rk2=False, mc=False, acc=None):
    """What the product's STAGE_ADVECT_VELOCITY leaves in utmp / vtmp (and in the dye fields): the transport - the oracle's own, tests/c/advect_rk2.c's
    or tests/c/advect_maccormack.c's -, the restated forcing, zero_bounds, and with viscosity the oracle's diffusion extension."""
    lib = o.lib
    dtc = C.c_float(dt)
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
        if o.c.rainbow:      # main.c:873-882: the memcpy moves the WHOLE tmp array
            for q, tmp in ((o.cr, o.crtmp), (o.cg, o.cgtmp), (o.cb, o.cbtmp)):
                lib.eo_advect_p(o.ptr, o.f32p(q), o.f32p(o.u), o.f32p(o.v), dtc, o.f32p(tmp))
                q[...] = tmp
    apply(o, f, boxes, t, dt, acc)      # (where eo_apply_body_forces stood)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.utmp), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.vtmp), V)
    if o.c.viscosity > 0.0:      # eo_substep's extension: u, v are its scratch
        _bind_diffuse(lib)
        lib.eo_diffuse(o.ptr, o.f32p(o.utmp), U, dtc, o.f32p(o.u))
        lib.eo_diffuse(o.ptr, o.f32p(o.vtmp), V, dtc, o.f32p(o.v))
        o.utmp[:, :-1] = o.u[:, :-1]
        o.vtmp[:-1, :] = o.v[:-1, :]


def substep(am, o, dt, f, boxes, clock, rk2=False, mc=False, acc_at=None):
    """eo_substep (main.c:855-898) with the forcing taken at the clock's time at the START of the substep; the clock advances behind it.
    acc_at(f, t) -> (ax, ay) replaces forcing_at.  Returns the PCG iterations."""
    lib = o.lib
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
    advect_velocity_stage(am, o, dt, f, boxes, clock.t, rk2, mc, None if acc_at is None else acc_at(f, clock.t))
    it = lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    o.c.total_substeps += 1
    o.c.last_dt = dt
    clock.advance(dt)
    return it


def step(am, o, f, boxes, clock, rk2=False, mc=False, acc_at=None, frame_time=0.1, max_substeps=8):
    """eo_step (main.c:843-853): CFL substeps until the frame time is used up, at most 8."""
    ft = F32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = F32(ft - dt)
        iters += substep(am, o, float(dt), f, boxes, clock, rk2, mc, acc_at)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return n, iters
