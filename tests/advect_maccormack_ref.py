"""Test-side restatement of the MacCormack transport (EULER_OPT_ADVECT_MACCORMACK, docs/advection_maccormack.md).

tests/c/advect_maccormack.c restates the velocity and dye stages over the oracle's exported eo_interpolate and eo_sim
arrays (with tests/c/advect_rk2.c's traces and marker move); it is compiled here, at test time, into a temporary directory
and linked against the in-tree liboracle.so.  `substep` / `step` compose a whole frame like advect_rk2_ref, with the new
velocity and dye stage swapped in.

Test infrastructure only: nothing under euler_amd/ imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import advect_rk2_ref as rk2ref
from oracle_lib import ORACLE_DIR, P, U, V, build_oracle, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "advect_maccormack.c")
_LIB = {}


def build(outdir):
    """Compile tests/c/advect_maccormack.c into outdir (once per process) and return the ctypes library.  It also carries the
    ar_* functions of tests/c/advect_rk2.c."""
    if "lib" in _LIB:
        return _LIB["lib"]
    build_oracle()
    so = os.path.join(str(outdir), "libadvect_maccormack.so")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-shared",
                           "-I" + ORACLE_DIR, "-I" + os.path.dirname(SRC), "-o", so, SRC, "-L" + ORACLE_DIR, "-loracle",
                           "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    oracle_lib()
    lib = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    for n in ("am_advect_u", "am_advect_v"):
        getattr(lib, n).argtypes = [C.c_void_p, fp, fp, C.c_float, fp, C.c_int, C.c_int, fp, fp]
    lib.am_advect_p.argtypes = [C.c_void_p, fp, fp, fp, C.c_float, fp, C.c_int, C.c_int, fp, fp]
    lib.ar_advect_u.argtypes = [C.c_void_p, fp, fp, C.c_float, fp, C.c_int]
    lib.ar_advect_v.argtypes = [C.c_void_p, fp, fp, C.c_float, fp, C.c_int]
    lib.ar_advect_p.argtypes = [C.c_void_p, fp, fp, fp, C.c_float, fp, C.c_int]
    lib.ar_advect_markers.argtypes = [C.c_void_p, C.c_float, C.c_int]
    lib.ar_advect_markers.restype = C.c_int
    _LIB["lib"] = lib
    return lib


def _p(o):
    return C.cast(o.ptr, C.c_void_p)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def advect_u(am, o, u, v, dt, out, rk2, mc, lo=None, hi=None):
    am.am_advect_u(_p(o), _fp(u), _fp(v), C.c_float(dt), _fp(out), int(rk2), int(mc), _fp(lo), _fp(hi))


def advect_v(am, o, u, v, dt, out, rk2, mc, lo=None, hi=None):
    am.am_advect_v(_p(o), _fp(u), _fp(v), C.c_float(dt), _fp(out), int(rk2), int(mc), _fp(lo), _fp(hi))


def advect_p(am, o, q, u, v, dt, tmp, rk2, mc, lo=None, hi=None):
    am.am_advect_p(_p(o), _fp(q), _fp(u), _fp(v), C.c_float(dt), _fp(tmp), int(rk2), int(mc), _fp(lo), _fp(hi))


def advect_velocity_stage(am, o, dt, rk2, mc):
    """What the product's STAGE_ADVECT_VELOCITY leaves in utmp / vtmp and the dye fields: the dye (forward result in *tmp, the corrected
    channel in r / g / b), then u / v, body forces, zero_bounds."""
    lib = o.lib
    if o.c.rainbow:
        for q, t in ((o.cr, o.crtmp), (o.cg, o.cgtmp), (o.cb, o.cbtmp)):
            advect_p(am, o, q, o.u, o.v, dt, t, rk2, mc)
    advect_u(am, o, o.u, o.v, dt, o.utmp, rk2, mc)
    advect_v(am, o, o.u, o.v, dt, o.vtmp, rk2, mc)
    lib.eo_apply_body_forces(o.ptr, o.f32p(o.vtmp), C.c_float(dt))
    lib.eo_zero_bounds(o.ptr, o.f32p(o.utmp), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.vtmp), V)


def substep(am, o, dt, rk2, mc):
    """eo_substep (main.c:855-898) with the transport steps restated; returns the PCG iterations."""
    lib = o.lib
    assert not (o.c.viscosity > 0.0), "the restatement composes the reference's inviscid substep"
    rk2ref.advect_markers(am, o, dt, rk2)
    lib.eo_refresh_marker_counts(o.ptr)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            lib.eo_extrapolate(o.ptr, o.f32p(q), P)
    lib.eo_update_fluid_sources(o.ptr)
    lib.eo_extrapolate(o.ptr, o.f32p(o.u), U)
    lib.eo_extrapolate(o.ptr, o.f32p(o.v), V)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.u), U)
    lib.eo_zero_bounds(o.ptr, o.f32p(o.v), V)
    advect_velocity_stage(am, o, dt, rk2, mc)
    it = lib.eo_project(o.ptr, C.c_float(dt), o.f32p(o.utmp), o.f32p(o.vtmp), o.f32p(o.u), o.f32p(o.v))
    o.c.total_substeps += 1
    o.c.last_dt = dt
    return it


def step(am, o, rk2, mc, frame_time=0.1, max_substeps=8):
    """eo_step (main.c:843-853): CFL substeps until the frame time is used up, at most 8."""
    ft = np.float32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = np.float32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = np.float32(ft - dt)
        iters += substep(am, o, float(dt), rk2, mc)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return n, iters


# ----------------------------------------------------------------------------- translation of a smooth bump (host and GPU tests)
TR_VEL = (0.37, 0.23)      # cells per step, dt = 1


def bump(n, t=0.0, amp=1.0):
    """a Gaussian (sigma = n / 16) on cell centres (index space), started at (0.35 n, 0.35 n) and carried t steps by TR_VEL"""
    ys, xs = np.indices((n, n)).astype(np.float64)
    cx, cy = 0.35 * n + TR_VEL[0] * t, 0.35 * n + TR_VEL[1] * t
    s = n / 16.0
    return amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * s * s))


def translation_box(n):
    """u, v (uniform TR_VEL), count (1 inside the border ring), sink (the ring)"""
    u = np.full((n, n), TR_VEL[0], np.float32)
    v = np.full((n, n), TR_VEL[1], np.float32)
    sink = np.zeros((n, n), np.uint8)
    sink[0, :] = sink[-1, :] = sink[:, 0] = sink[:, -1] = 1
    return u, v, (1 - sink).astype(np.uint8), sink


def rel_l2(got, want):
    got = got.astype(np.float64)
    return float(np.sqrt(((got - want) ** 2).sum() / (want ** 2).sum()))


def vbump(n, t=0.0, amp=0.05):
    """the velocity check: v = 0.23 + a bump in x alone (sigma = n / 16), on the v faces' x index; carried by u = 0.37 only (v does not vary in y)"""
    xs = np.indices((n, n))[1].astype(np.float64)
    cx, s = 0.35 * n + TR_VEL[0] * t, n / 16.0
    return TR_VEL[1] + amp * np.exp(-((xs - cx) ** 2) / (2 * s * s))
