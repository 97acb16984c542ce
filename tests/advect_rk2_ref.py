"""Test-side restatement of the midpoint (RK2) transport (EULER_OPT_ADVECT_RK2, docs/advection_rk2.md).

tests/c/advect_rk2.c restates the four transport steps over the oracle's exported eo_interpolate and
eo_sim arrays; it is compiled here, at test time, into a temporary directory and linked against the
in-tree liboracle.so.  `substep` / `step` compose a whole frame in the order of the reference's
sim_step (main.c:843-900), with every other stage taken from the oracle unchanged.

Test infrastructure only: nothing under euler_amd/ imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle_lib import ORACLE_DIR, P, U, V, build_oracle, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "advect_rk2.c")
_LIB = {}


def build(outdir):
    """Compile tests/c/advect_rk2.c into outdir (once per process) and return the ctypes library."""
    if "lib" in _LIB:
        return _LIB["lib"]
    build_oracle()
    so = os.path.join(str(outdir), "libadvect_rk2.so")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-shared",
                           "-I" + ORACLE_DIR, "-o", so, SRC, "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    oracle_lib()      # the oracle's own bindings first: the restatement runs on the same eo_sim
    lib = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    lib.ar_advect_u.argtypes = [C.c_void_p, fp, fp, C.c_float, fp, C.c_int]
    lib.ar_advect_v.argtypes = [C.c_void_p, fp, fp, C.c_float, fp, C.c_int]
    lib.ar_advect_p.argtypes = [C.c_void_p, fp, fp, fp, C.c_float, fp, C.c_int]
    lib.ar_advect_markers.argtypes = [C.c_void_p, C.c_float, C.c_int]
    lib.ar_advect_markers.restype = C.c_int
    _LIB["lib"] = lib
    return lib


def _p(o):
    return C.cast(o.ptr, C.c_void_p)


def advect_markers(ar, o, dt, rk2):
    """The marker move (eo_advect_markers with the midpoint); returns the dt-shortening collisions."""
    return ar.ar_advect_markers(_p(o), C.c_float(dt), int(rk2))


def advect_velocity_stage(ar, o, dt, rk2):
    """What the product's STAGE_ADVECT_VELOCITY leaves in utmp / vtmp (and in the dye fields):
    advect_u / advect_v (+ advect_p and the whole-array copy with the dye), body forces, zero_bounds."""
    lib = o.lib
    dt = C.c_float(dt)
    ar.ar_advect_u(_p(o), o.f32p(o.u), o.f32p(o.v), dt, o.f32p(o.utmp), int(rk2))
    ar.ar_advect_v(_p(o), o.f32p(o.u), o.f32p(o.v), dt, o.f32p(o.vtmp), int(rk2))
    if o.c.rainbow:      # main.c:873-882: the memcpy moves the WHOLE tmp array
        for q, t in ((o.cr, o.crtmp), (o.cg, o.cgtmp), (o.cb, o.cbtmp)):
            ar.ar_advect_p(_p(o), o.f32p(q), o.f32p(o.u), o.f32p(o.v), dt, o.f32p(t), int(rk2))
            q[...] = t
    lib.eo_apply_body_forces(o.ptr, o.f32p(o.vtmp), dt)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.utmp), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.vtmp), V)


def substep(ar, o, dt, rk2):
    """eo_substep (main.c:855-898) with the transport steps restated; returns the PCG iterations."""
    lib = o.lib
    assert not (o.c.viscosity > 0.0), "the restatement composes the reference's inviscid substep"
    advect_markers(ar, o, dt, rk2)
    lib.eo_refresh_marker_counts(o.ptr)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            lib.eo_extrapolate(o.ptr, o.f32p(q), P)
    lib.eo_update_fluid_sources(o.ptr)
    lib.eo_extrapolate(o.ptr, o.f32p(o.u), U)
    lib.eo_extrapolate(o.ptr, o.f32p(o.v), V)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.u), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.v), V)
    advect_velocity_stage(ar, o, dt, rk2)
    it = lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    o.c.total_substeps += 1
    o.c.last_dt = dt
    return it


def step(ar, o, rk2, frame_time=0.1, max_substeps=8):
    """eo_step (main.c:843-853): CFL substeps until the frame time is used up, at most 8."""
    ft = np.float32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = np.float32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = np.float32(ft - dt)
        iters += substep(ar, o, float(dt), rk2)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return n, iters


# ----------------------------------------------------------------------------- the analytic rotation (host and GPU tests)
ROT_N = 48            # grid cells per side, all fluid inside the sink ring
ROT_C = 24.0          # the centre of rotation (a position)
ROT_CORE = 6.0        # rigid rotation for |offset| <= ROT_CORE per axis, the velocity held constant beyond: the CFL dt follows the core's speeds,
                      # which keeps the turn per step (~0.09 rad) large enough that the RK2 error stays far above float32 rounding
ROT_OMEGA = 1.0


def rotation_fields(n=ROT_N, c=ROT_C, core=ROT_CORE, omega=ROT_OMEGA):
    """u, v on their faces (u face (x, y) at position (x + 1, y + 0.5), v face at (x + 0.5, y + 1)) of the rotation about (c, c),
    count (1 inside the border ring), sink (the border ring)."""
    ys, xs = np.indices((n, n)).astype(np.float64)
    u = (-omega * np.clip(ys + 0.5 - c, -core, core)).astype(np.float32)
    v = (omega * np.clip(xs + 0.5 - c, -core, core)).astype(np.float32)
    u[:, -1] = 0
    v[-1, :] = 0
    sink = np.zeros((n, n), np.uint8)
    sink[0, :] = sink[-1, :] = sink[:, 0] = sink[:, -1] = 1
    count = (1 - sink).astype(np.uint8)
    return u, v, count, sink


def rotation_test_faces(n=ROT_N, c=ROT_C, reach=ROT_CORE - 2.5):      # (displacement <= 0.35, the stencil one cell beyond: inside the core)
    """u faces whose back-trace and its bilinear stencil stay inside the rigid core: (ys, xs, position x, position y)"""
    ys, xs = np.indices((n, n - 1))
    px, py = xs + 1.0, ys + 0.5
    r = np.hypot(px - c, py - c)
    sel = (r <= reach) & (r >= 1.0)
    return ys[sel], xs[sel], px[sel], py[sel]


def rotation_u_error(utmp, dt, c=ROT_C, omega=ROT_OMEGA):
    """max |advected u - exact| over the test faces: the exact frozen-field back-trace of a rigid rotation is the position
    rotated by -omega dt; u there is -omega (y' - c)"""
    ys, xs, px, py = rotation_test_faces()
    th = -omega * float(dt)
    qy = c + np.sin(th) * (px - c) + np.cos(th) * (py - c)
    exact = -omega * (qy - c)
    return float(np.abs(utmp[ys, xs].astype(np.float64) - exact).max())


def rotation_markers(c=ROT_C, r=3.0, k=32):
    a = np.arange(k) * (2 * np.pi / k) + 0.1
    return np.stack([c + r * np.cos(a), c + r * np.sin(a)], 1).astype(np.float32)


def radius_drift(m, c=ROT_C, r=3.0):
    return float(np.abs(np.hypot(m[:, 0].astype(np.float64) - c, m[:, 1].astype(np.float64) - c) - r).mean())
