"""Test-side restatement of the moving bodies (euler_set_bodies, include/euler.h, docs/bodies.md): solid boxes that push water at a prescribed velocity.

Written from the header's rules, not from the kernels: the yardstick of test_bodies_host.py and test_gpu_bodies.py.
  body / body_at      a body as a dict, the law of motion in numpy doubles: clamp, floor(px + 0.5)
  targets             per body the target origin at t + dt and the substep's wall velocity (float32)
  plan                the unit shifts from an origin to a target: all x shifts first, then y
  set_bodies          switching on: the old rectangles cleared, the new ones made solid as EULER_EDIT_SOLID does (markers inside deleted, edit_ref's removal)
  begin_arrays        the shifts of one substep on plain arrays, numpy: the push, the strips' masks, every rectangle solid again
  begin_loops         the same in plain Python loops, marker by marker and cell by cell (a second restatement)
  begin               begin_arrays on an oracle's arrays
  impose / withdraw   the wall velocity on utmp / vtmp in front of the projection, and the zeros behind it
  substep / step      compose a substep as forcing_ref does, over the oracle's exported stage functions, with the bodies and a double clock; heat = (T, record,
                      boxes) composes it over heat_ref's stages instead, with the dry cells at ambient right behind a shift

A body is a dict with the keys of FIELDS; origins is a list of [ox, oy], one per body, changed in place.  `at` replaces body_at where a test takes the positions
from euler_body_at itself, so that no libm difference reaches it.
Test infrastructure only: nothing under euler_amd/ imports this module."""
import ctypes as C

import numpy as np

import forcing_ref as fref
import heat_ref as href

FIELDS = ("x", "y", "hz", "phase", "vx", "vy", "amp_x", "amp_y", "w", "h")
F32 = np.float32
F64 = np.float64


def body(size, at, velocity=(0.0, 0.0), amplitude=(0.0, 0.0), hz=0.0, phase=0.0):
    return dict(w=int(size[0]), h=int(size[1]), x=float(at[0]), y=float(at[1]), vx=float(F32(velocity[0])), vy=float(F32(velocity[1])),
                amp_x=float(F32(amplitude[0])), amp_y=float(F32(amplitude[1])), hz=float(hz), phase=float(phase))


def body_at(b, t, X, Y):
    """-> (px, py, ox, oy): in double, p = x + vx t + amp sin(2 pi hz t + phase), clamped to [2, X - 2 - w], the origin floor(px + 0.5)"""
    s = np.sin(F64(2.0 * np.pi) * F64(b["hz"]) * F64(t) + F64(b["phase"]))
    px = F64(b["x"]) + F64(F32(b["vx"])) * F64(t) + F64(F32(b["amp_x"])) * s
    py = F64(b["y"]) + F64(F32(b["vy"])) * F64(t) + F64(F32(b["amp_y"])) * s
    px = min(max(px, F64(2)), F64(X - 2 - b["w"]))
    py = min(max(py, F64(2)), F64(Y - 2 - b["h"]))
    return float(px), float(py), int(np.floor(px + 0.5)), int(np.floor(py + 0.5))


def targets(bodies, t, dt, X, Y, at=body_at):
    """-> [(tx, ty, wx, wy)]: the origin at t + dt; the mean velocity over the substep, (float)((p(t + dt) - p(t)) / (double)dt)"""
    out = []
    dtd = F64(F32(dt))
    t1 = float(F64(t) + dtd)
    for b in bodies:
        px0, py0, _, _ = at(b, t, X, Y)
        px1, py1, tx, ty = at(b, t1, X, Y)
        out.append((tx, ty, F32((F64(px1) - F64(px0)) / dtd), F32((F64(py1) - F64(py0)) / dtd)))
    return out


def plan(ox, oy, tx, ty):
    """the unit shifts (axis, dir) from (ox, oy) to (tx, ty): all of x first, then y"""
    sx, sy = (1 if tx > ox else -1), (1 if ty > oy else -1)
    return [(0, sx)] * abs(tx - ox) + [(1, sy)] * abs(ty - oy)


def strips(ox, oy, w, h, axis, d):
    """-> (fill, clear): the strip ahead of the moving face and the one behind the body, inclusive boxes (x0, y0, x1, y1), for the body at (ox, oy) before the shift"""
    if axis == 0:
        xf, xc = (ox + w, ox) if d > 0 else (ox - 1, ox + w - 1)
        return (xf, oy, xf, oy + h - 1), (xc, oy, xc, oy + h - 1)
    yf, yc = (oy + h, oy) if d > 0 else (oy - 1, oy + h - 1)
    return (ox, yf, ox + w - 1, yf), (ox, yc, ox + w - 1, yc)


def _sl(box):
    x0, y0, x1, y1 = box
    return (slice(y0, y1 + 1), slice(x0, x1 + 1))


def solid_cells(solid, source, sink, count, box):
    """the masks and the count of EULER_EDIT_SOLID over the box (tests/edit_ref.py: solid = 1, source = sink = 0, count = 0); the markers are the caller's"""
    sl = _sl(box)
    solid[sl], source[sl], sink[sl], count[sl] = 1, 0, 0, 0


def clear_cells(solid, source, sink, box):
    """the mask change of EULER_EDIT_CLEAR"""
    sl = _sl(box)
    solid[sl], source[sl], sink[sl] = 0, 0, 0


def rect(b, origin):
    return (origin[0], origin[1], origin[0] + b["w"] - 1, origin[1] + b["h"] - 1)


# ----------------------------------------------------------------------------- the shifts of a substep: numpy
def begin_arrays(markers, solid, source, sink, count, bodies, origins, tgt):
    """In place.  markers: (n, 2) float32.  -> the number of unit shifts.  The counts of the cells the markers land in are NOT updated."""
    shifts = 0
    for b, o, (tx, ty, _, _) in zip(bodies, origins, tgt):
        for axis, d in plan(o[0], o[1], tx, ty):
            fill, clear = strips(o[0], o[1], b["w"], b["h"], axis, d)
            fx, fy = np.floor(markers[:, 0]), np.floor(markers[:, 1])
            hit = (fill[0] <= fx) & (fx <= fill[2]) & (fill[1] <= fy) & (fy <= fill[3])
            markers[hit, axis] = markers[hit, axis] + F32(d)
            solid_cells(solid, source, sink, count, fill)
            clear_cells(solid, source, sink, clear)
            o[axis] += d
            shifts += 1
    if shifts:
        for b, o in zip(bodies, origins):
            solid_cells(solid, source, sink, count, rect(b, o))
    return shifts


# ----------------------------------------------------------------------------- ... and in plain loops
def begin_loops(markers, solid, source, sink, count, bodies, origins, tgt):
    shifts = 0
    for k in range(len(bodies)):
        w, h = bodies[k]["w"], bodies[k]["h"]
        tx, ty = tgt[k][0], tgt[k][1]
        while origins[k][0] != tx or origins[k][1] != ty:
            ox, oy = origins[k]
            if ox != tx:      # x until it is done
                d = 1 if tx > ox else -1
                col = ox + w if d > 0 else ox - 1
                for i in range(len(markers)):
                    if np.floor(markers[i, 0]) == col and oy <= np.floor(markers[i, 1]) <= oy + h - 1:
                        markers[i, 0] = F32(markers[i, 0] + F32(d))
                gone = ox if d > 0 else ox + w - 1
                for y in range(oy, oy + h):
                    solid[y, col], source[y, col], sink[y, col], count[y, col] = 1, 0, 0, 0
                for y in range(oy, oy + h):
                    solid[y, gone], source[y, gone], sink[y, gone] = 0, 0, 0
                origins[k][0] = ox + d
            else:
                d = 1 if ty > oy else -1
                row = oy + h if d > 0 else oy - 1
                for i in range(len(markers)):
                    if np.floor(markers[i, 1]) == row and ox <= np.floor(markers[i, 0]) <= ox + w - 1:
                        markers[i, 1] = F32(markers[i, 1] + F32(d))
                gone = oy if d > 0 else oy + h - 1
                for x in range(ox, ox + w):
                    solid[row, x], source[row, x], sink[row, x], count[row, x] = 1, 0, 0, 0
                for x in range(ox, ox + w):
                    solid[gone, x], source[gone, x], sink[gone, x] = 0, 0, 0
                origins[k][1] = oy + d
            shifts += 1
    if shifts:
        for k in range(len(bodies)):
            ox, oy = origins[k]
            for y in range(oy, oy + bodies[k]["h"]):
                for x in range(ox, ox + bodies[k]["w"]):
                    solid[y, x], source[y, x], sink[y, x], count[y, x] = 1, 0, 0, 0
    return shifts


def begin(o, bodies, origins, t, dt, at=body_at):
    """The bodies' work in front of the marker advection of a substep of step dt at clock t, on the oracle's arrays.  -> the number of unit shifts."""
    return begin_arrays(o.markers, o.solid, o.source, o.sink, o.count, bodies, origins, targets(bodies, t, dt, o.X, o.Y, at))


# ----------------------------------------------------------------------------- switching on
def delete_in_box(markers, box):
    """refresh_marker_counts' removal with "in the box" as its condition (tests/edit_ref.py delete_in_box_vectorised, restated here so that this module needs no GPU package)"""
    m = np.array(markers, F32).reshape(-1, 2)
    x0, y0, x1, y1 = box
    fx, fy = np.floor(m[:, 0]), np.floor(m[:, 1])
    gone = (x0 <= fx) & (fx <= x1) & (y0 <= fy) & (fy <= y1)
    n1 = len(m) - int(gone.sum())
    out = m[:n1].copy()
    out[np.nonzero(gone[:n1])[0]] = m[n1:][~gone[n1:]][::-1]
    return out


def set_bodies(o, old, old_origins, new, t, at=body_at):
    """euler_set_bodies at clock t on the oracle: -> the new origins"""
    for b, og in zip(old, old_origins):
        clear_cells(o.solid, o.source, o.sink, rect(b, og))
    origins = []
    for b in new:
        _, _, ox, oy = at(b, t, o.X, o.Y)
        origins.append([ox, oy])
        box = rect(b, origins[-1])
        o.set_markers(delete_in_box(o.markers, box))
        solid_cells(o.solid, o.source, o.sink, o.count, box)
    return origins


# ----------------------------------------------------------------------------- the wall velocity
def _faces(utmp, vtmp, solid, count, bodies, origins, tgt, value):
    """bodies in list order; value(w) is what a face whose rule fires takes"""
    wet = (np.asarray(count) != 0) & (np.asarray(solid) == 0)
    for b, (ox, oy), (_, _, wx, wy) in zip(bodies, origins, tgt):
        w, h = b["w"], b["h"]
        if wx != F32(0):
            for y in range(oy, oy + h):
                if wet[y, ox - 1]:
                    utmp[y, ox - 1] = value(wx)      # the left edge: the face between cell ox - 1 and the body
                if wet[y, ox + w]:
                    utmp[y, ox + w - 1] = value(wx)  # the right edge
        if wy != F32(0):
            for x in range(ox, ox + w):
                if wet[oy - 1, x]:
                    vtmp[oy - 1, x] = value(wy)
                if wet[oy + h, x]:
                    vtmp[oy + h - 1, x] = value(wy)


def impose(o, bodies, origins, tgt):
    _faces(o.utmp, o.vtmp, o.solid, o.count, bodies, origins, tgt, lambda w: F32(w))


def withdraw(o, bodies, origins, tgt):
    _faces(o.utmp, o.vtmp, o.solid, o.count, bodies, origins, tgt, lambda w: F32(0))


def project_stage(o, dt, bodies, origins, tgt):
    """EULER_STAGE_PROJECT with bodies -> the PCG iterations"""
    impose(o, bodies, origins, tgt)
    it = o.lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    withdraw(o, bodies, origins, tgt)
    return it


# ----------------------------------------------------------------------------- the composition
def substep(am, o, dt, bodies, origins, clock, f=None, boxes=(), rk2=False, mc=False, acc_at=None, at=body_at, heat=None):
    """forcing_ref.substep with the bodies: their shifts in front of the marker advection, their wall velocity around the projection, all at the clock's
    time at the START of the substep; the clock advances behind it.  heat = (T, record, boxes): the temperature's two stages as heat_ref.substep has them, and
    behind a shift every cell without markers holds ambient.  Returns the PCG iterations."""
    lib = o.lib
    tgt = targets(bodies, clock.t, dt, o.X, o.Y, at)
    shifts = begin_arrays(o.markers, o.solid, o.source, o.sink, o.count, bodies, origins, tgt)
    if heat is not None and shifts:
        heat[0][np.asarray(o.count) == 0] = F32(dict(href.DEFAULT, **heat[1])["ambient"])
    if rk2:
        am.ar_advect_markers(C.cast(o.ptr, C.c_void_p), C.c_float(dt), 1)
    else:
        lib.eo_advect_markers(o.ptr, C.c_float(dt))
    lib.eo_refresh_marker_counts(o.ptr)
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
    it = project_stage(o, dt, bodies, origins, tgt)
    o.c.total_substeps += 1
    o.c.last_dt = dt
    clock.advance(dt)
    return it


def step(am, o, bodies, origins, clock, f=None, boxes=(), rk2=False, mc=False, acc_at=None, at=body_at, frame_time=0.1, max_substeps=8, heat=None):
    """eo_step (main.c:843-853) over substep above"""
    ft = F32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = F32(ft - dt)
        iters += substep(am, o, float(dt), bodies, origins, clock, f, boxes, rk2, mc, acc_at, at, heat)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return n, iters
