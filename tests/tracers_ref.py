"""Test-side restatement of the passive tracers (docs/tracers.md, include/euler.h euler_tracer).

`tracer_substep` runs the rules of one substep in np.float32 over an array of TRACER_DTYPE records; the walk itself (rule 4) is the oracle-side marker
walk on a ONE-MARKER array per tracer (tests/c/tracers_walk.c over tests/c/advect_rk2.c), never several tracers in one marker array: the dt chain would
couple them.  `substep` / `step` compose a frame over advect_rk2_ref / advect_maccormack_ref with the tracers moved first, as the product's launch comes
in front of the marker launches.  The raster and the painter are numpy integers.

Test infrastructure only: nothing under euler_amd/ imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import advect_maccormack_ref as mcref
import advect_rk2_ref as rk2ref
import euler_amd as ea
from oracle_lib import ORACLE_DIR, build_oracle, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "tracers_walk.c")
F32 = np.float32
_LIB = {}


def build(outdir):
    """(am, tw): the MacCormack / RK2 restatement's library (advect_maccormack_ref.build) and tests/c/tracers_walk.c compiled into outdir, once per process."""
    if "libs" in _LIB:
        return _LIB["libs"]
    am = mcref.build(outdir)
    build_oracle()
    so = os.path.join(str(outdir), "libtracers_walk.so")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-shared",
                           "-I" + ORACLE_DIR, "-I" + os.path.dirname(SRC), "-o", so, SRC, "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    oracle_lib()
    tw = C.CDLL(so)
    tw.tr_walk.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_float, C.c_int]
    tw.tr_walk.restype = None
    tw.ar_advect_markers.argtypes = [C.c_void_p, C.c_float, C.c_int]
    tw.ar_advect_markers.restype = C.c_int
    _LIB["libs"] = (am, tw)
    return _LIB["libs"]


def records(xy):
    """fresh records at the positions xy: all other words 0"""
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    rec = np.zeros(len(xy), ea.TRACER_DTYPE)
    rec["x"], rec["y"] = xy[:, 0], xy[:, 1]
    return rec


def walk(tw, o, xy, dt, rk2):
    """rule 4: every position through the one-marker walk with the full dt; the oracle's own markers stay as they are"""
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2).copy()
    if len(xy):
        tw.tr_walk(C.cast(o.ptr, C.c_void_p), xy.ctypes.data_as(C.POINTER(C.c_float)), len(xy), C.c_float(dt), int(rk2))
    return xy


def tracer_substep(tw, o, rec, dt, rk2):
    """one substep of every record, in place (rules 1-6 of include/euler.h), reading the oracle's u, v, count, solid, sink as they stand"""
    dt = F32(dt)
    X, Y = o.X, o.Y
    x, y = rec["x"].copy(), rec["y"].copy()
    live = (rec["flags"] & ea.TRACER_RETIRED) == 0
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        inside = np.isfinite(x) & np.isfinite(y) & (fx >= 0) & (fx <= X - 1) & (fy >= 0) & (fy <= Y - 1)
    lost = live & ~inside
    rec["flags"][lost] |= ea.TRACER_RETIRED | ea.TRACER_LOST
    cx = np.where(inside, fx, 0).astype(np.int64)
    cy = np.where(inside, fy, 0).astype(np.int64)
    here = live & inside
    in_solid = here & (o.solid[cy, cx] != 0)
    in_sink = here & ~in_solid & (o.sink[cy, cx] != 0)
    rec["flags"][in_solid] |= ea.TRACER_RETIRED | ea.TRACER_IN_SOLID
    rec["flags"][in_sink] |= ea.TRACER_RETIRED | ea.TRACER_IN_SINK
    go = here & ~in_solid & ~in_sink
    if not go.any():
        return rec
    wet = o.count[cy, cx] != 0
    new = walk(tw, o, np.stack([x[go], y[go]], 1), dt, rk2)
    dx, dy = new[:, 0] - x[go], new[:, 1] - y[go]
    assert dx.dtype == F32 and dt.dtype == F32
    rec["path"][go] = rec["path"][go] + np.sqrt(dx * dx + dy * dy)      # (np.sqrt on float32: correctly rounded)
    rec["age"][go] = rec["age"][go] + dt
    gw = go & wet
    rec["wet_time"][gw] = rec["wet_time"][gw] + dt
    rec["substeps"][go] += 1
    rec["flags"][gw] |= ea.TRACER_WET
    gd = go & ~wet
    rec["flags"][gd] = (rec["flags"][gd] & ~np.uint32(ea.TRACER_WET)) | ea.TRACER_WAS_DRY
    rec["x"][go], rec["y"][go] = new[:, 0], new[:, 1]
    return rec


def substep(libs, o, rec, dt, rk2=False, mc=False):
    """the tracers first, then the substep of the restatement; returns the PCG iterations"""
    am, tw = libs
    tracer_substep(tw, o, rec, dt, rk2)
    return mcref.substep(am, o, dt, rk2, mc) if mc else rk2ref.substep(am, o, dt, rk2)


def step(libs, o, rec, rk2=False, mc=False, clock=0.0, frame_time=0.1, max_substeps=8):
    """eo_step (main.c:843-853) over `substep`; returns the clock advanced by (double)dt per substep, as euler_get_time counts"""
    ft = F32(frame_time)
    iters = n = 0
    while ft > 0 and n < max_substeps:
        dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
        ft = F32(ft - dt)
        iters += substep(libs, o, rec, float(dt), rk2, mc)
        clock += float(dt)
        n += 1
    o.c.last_substeps = n
    o.c.last_pcg_iterations = iters
    o.c.frame_count += 1
    return clock


# ----------------------------------------------------------------------------- the raster and the painter
def pixel(c, B, W):
    """the pixel of euler_overview_box's geometry that covers column c of a box of B columns shown as W pixels (rows alike, from the top)"""
    return ((np.asarray(c, np.int64) + 1) * W - 1) // B


def pixel_brute(c, B, W):
    """... by the covering definition: pixel p covers the columns floor(p B / W) ... floor((p + 1) B / W) - 1"""
    hit = [p for p in range(W) if (p * B) // W <= c <= ((p + 1) * B) // W - 1]
    assert len(hit) == 1, (c, B, W, hit)
    return hit[0]


def raster(rec, box, W, H, all=False):
    x0, y0, x1, y1 = box
    Bw, Bh = x1 - x0 + 1, y1 - y0 + 1
    x, y = rec["x"], rec["y"]
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        sel = np.isfinite(x) & np.isfinite(y) & (fx >= x0) & (fx <= x1) & (fy >= y0) & (fy <= y1)
    if not all:
        sel &= (rec["flags"] & ea.TRACER_RETIRED) == 0
    out = np.zeros((H, W), np.uint32)
    c = fx[sel].astype(np.int64) - x0
    r = y1 - fy[sel].astype(np.int64)
    np.add.at(out, (pixel(r, Bh, H), pixel(c, Bw, W)), 1)
    return out


def q24(v):
    v = F32(v)
    c = v if v > 0 else F32(0)      # (a NaN: 0)
    c = F32(1) if c > 1 else c
    return int(np.uint32(c * F32(16777216.0)))


def paint(counts, px, fg, bg=None):
    px = px.copy()
    water = px["water"].astype(np.uint64)
    wet = px["water"] > 0
    on = wet & (counts > 0)
    off = wet & (counts == 0)
    for c in range(3):
        d = px["dye"][..., c]
        d[on] = water[on] * np.uint64(q24(fg[c]))
        if bg is not None:
            d[off] = water[off] * np.uint64(q24(bg[c]))
    return px
