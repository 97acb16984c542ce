"""Plain CPU helpers for the capped-iterate tests of the resident solver (test_gpu_resident_iterates.py; checked themselves in test_resident_ref_host.py):
random walled scenes, b - A p in long double from the cell-mask encoding, a moving state to teacher-force a handle and a second oracle from, and the
oracle's tile-local solve (tile_records = 16, sequential sums) cut off after k iterations.

Test infrastructure only: nothing here touches the GPU library."""
import collections
import functools

import numpy as np

from euler_amd import scenarios
from golden_util import load, scenario_text
from oracle_lib import Oracle

STATE_GRIDS = ("solid", "source", "sink", "count", "prev_count", "u", "v", "utmp", "vtmp", "precon")
Capped = collections.namedtuple("Capped", "p iterations dt count r b residual cellmask")


def random_scene_text(seed, W=44, H=36):
    """Random walls, pools and air pockets: 10 % walls, 52 % water, the rest air, a closed border.  Upscaled to 300 x 260: chunks and aggregates without fluid,
    chunks cut by walls, fluid in single cells, pools closed off from each other."""
    rng = np.random.default_rng(seed)
    rows = []
    for y in range(H):
        r = rng.random(W)
        row = "".join("X" if v < 0.10 else ("0" if v < 0.62 else " ") for v in r)
        rows.append("X" + row[1:-1] + "X")
    rows[0] = rows[-1] = "X" * W
    return "\n".join(rows) + "\n"


def true_residual(b, p, cellmask):
    """b - A p on the fluid cells (0 elsewhere) in long double, A from the cell-mask encoding: bit 0 fluid, bits 1..4 fluid at x+1, y+1, x-1, y-1,
    bits 5.. the diagonal."""
    m = np.asarray(cellmask)
    pl = np.asarray(p, np.longdouble)
    ap = (m >> 5).astype(np.longdouble) * pl
    ap[:, :-1] -= np.where((m[:, :-1] & 2) != 0, pl[:, 1:], 0)
    ap[:-1, :] -= np.where((m[:-1, :] & 4) != 0, pl[1:, :], 0)
    ap[:, 1:] -= np.where((m[:, 1:] & 8) != 0, pl[:, :-1], 0)
    ap[1:, :] -= np.where((m[1:, :] & 16) != 0, pl[:-1, :], 0)
    return np.where((m & 1) != 0, np.asarray(b, np.longdouble) - ap, 0)


def oracle_cellmask(o):
    """the cell-mask encoding of the system an oracle has just assembled (eo_build_system: fluid = count != 0, a_diag)"""
    fl = np.asarray(o.count) != 0
    m = fl.astype(np.uint8)
    m[:, :-1] |= (fl[:, 1:] << 1).astype(np.uint8)
    m[:-1, :] |= (fl[1:, :] << 2).astype(np.uint8)
    m[:, 1:] |= (fl[:, :-1] << 3).astype(np.uint8)
    m[1:, :] |= (fl[:-1, :] << 4).astype(np.uint8)
    m |= (np.asarray(o.a_diag).astype(np.uint8) << 5)
    return np.where(fl, m, 0).astype(np.uint8)


def unclamped(p, cellmask):
    """The fluid cells whose row of b - A p is untouched by the clamp that follows every solve (p < 0 -> 0, main.c:773-779): the pressure a caller reads is the
    clamped one, so a cell that reads 0, and every cell that has one as a fluid neighbour, is left out.  -> (kept cells, share of the fluid cells left out)"""
    m = np.asarray(cellmask)
    fl = (m & 1) != 0
    zero = fl & (np.asarray(p) == 0)
    hit = zero.copy()
    hit[:, :-1] |= zero[:, 1:] & ((m[:, :-1] & 2) != 0)
    hit[:-1, :] |= zero[1:, :] & ((m[:-1, :] & 4) != 0)
    hit[:, 1:] |= zero[:, :-1] & ((m[:, 1:] & 8) != 0)
    hit[1:, :] |= zero[:-1, :] & ((m[1:, :] & 16) != 0)
    keep = fl & ~hit
    return keep, float((fl & hit).sum()) / max(int(fl.sum()), 1)


def _tile_oracle(X, Y):
    o = Oracle(X, Y)
    o.c.tile_records = 16
    return o


def moving_state(X, Y, text, frames, upscale=True, stir=None):
    """The oracle (reference-identical sequential dots, tile_records = 16) stepped `frames` frames from `text`, so that u and v are not at rest: the arrays a
    handle and a second oracle are loaded from (frames = 0: the scene as loaded).  stir = a seed: u and v are then overwritten with uniform values of
    [-1, 1) - a scene whose water only ever falls freely (a uniform velocity field: b = 0, no solve at all) gets a right-hand side that way."""
    o = _tile_oracle(X, Y).load_text(text, upscale=upscale)
    for _ in range(frames):
        o.step()
    if stir is not None:
        rng = np.random.default_rng(stir)
        o.u[...] = rng.uniform(-1.0, 1.0, (Y, X)).astype(np.float32)
        o.v[...] = rng.uniform(-1.0, 1.0, (Y, X)).astype(np.float32)
    st = {n: np.array(getattr(o, n)) for n in STATE_GRIDS}
    st["markers"] = np.array(o.markers)
    st["rng_state"] = int(o.c.rng_state)
    st["source_exhausted"] = int(o.c.source_exhausted)
    st["X"], st["Y"] = X, Y
    o.close()
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


def oracle_from_state(state):
    o = _tile_oracle(state["X"], state["Y"])
    for n in STATE_GRIDS:
        getattr(o, n)[...] = state[n]
    o.set_markers(state["markers"])
    o.c.rng_state = state["rng_state"]
    o.c.source_exhausted = state["source_exhausted"]
    return o


def oracle_capped(state, k, f32=False):
    """One timestep + substep of the oracle from `state` with tile_records = 16, max_iterations = k, tol = 0 (pcg_f32 as asked) -> p (clamped, as every caller
    reads it), the iteration count and dt; besides them the cell grid, the solve's own r and b, its last residual and the system's cell mask."""
    o = oracle_from_state(state)
    o.c.max_iterations = k
    o.c.tol = 0.0
    o.c.pcg_f32 = int(f32)
    dt = o.timestep(0.1)
    it = o.substep(dt)
    out = Capped(np.array(o.p), int(it), dt, np.array(o.count), np.array(o.r), np.array(o.b), float(o.c.last_residual), oracle_cellmask(o))
    o.close()
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ----------------------------------------------------------------------------- the scenes of the capped-iterate tests
# name -> (X, Y, text, upscale, frames the oracle runs before the compared substep, stir).  The frames are chosen with the oracle alone (test_resident_ref_host.py
# holds every scene to what the GPU tests need of it): a right-hand side that is not zero - the weird-edges water and the dam break's block fall freely at first, b = 0
# or p <= 0 everywhere - and pressures that are not all clamped away.  The water of the three smallest scenes falls out of the grid without ever meeting anything
# (b = 0 in every frame): they are stirred instead.
def _scenes():
    sc = {}
    for seed in (1, 2, 3):
        sc["random%d" % seed] = (300, 260, random_scene_text(seed), True, 3, None)
    sc["weird_edges_257x129"] = (257, 129, scenario_text(load("weird-edges_frames.npz")), True, 22, None)      # width no multiple of a chunk, height ending inside a band
    sc["dam_break_65x300"] = (65, 300, scenarios.dam_break(), True, 56, None)                                    # one chunk column, five bands
    sc["two_by_two_8x8"] = (8, 8, "00\n00\n", False, 0, 8)                                                      # one chunk in all: three waves of the workgroup are inactive
    sc["flat_70x9"] = (70, 9, "0" * 68 + "\n" + "0" * 68 + "\n", False, 0, 70)
    sc["narrow_9x200"] = (9, 200, "\n".join(["0000000"] * 150) + "\n", False, 0, 9)                             # a band that is mostly skew padding
    return sc


SCENES = _scenes()
RANDOM = ["random1", "random2", "random3"]
DEGENERATE = ["two_by_two_8x8", "flat_70x9", "narrow_9x200"]
WALLED = [n for n in SCENES if n not in DEGENERATE]      # random, ragged, dam break
ITERATE_CAPS = (1, 2, 3, 5, 17)
RESIDUAL_CAPS = (1, 5, 40)
CLAMP_CAP = 0.05


def caps(name, all_caps):
    """The caps at which `name` still has a PCG iteration to show.  The stirred 8 x 8 grid holds four fluid cells: CG has solved that system after four iterations,
    p stops changing, and with tol = 0 the iterations beyond divide 0 by 0 sooner or later (the oracle: NaN from iteration 29 on) - it is compared at k = 1, 2, 3.
    The 70 x 9 grid's 136 cells are solved to the last bit before iteration 40."""
    if name == "two_by_two_8x8":
        return tuple(k for k in all_caps if k <= 3)
    if name == "flat_70x9":
        return tuple(k for k in all_caps if k <= 17)
    return tuple(all_caps)


ITERATE_CASES = [(n, k) for n in SCENES for k in caps(n, ITERATE_CAPS)]
F32_CASES = [(n, k) for n in WALLED for k in ITERATE_CAPS]
# The pressure a caller reads is clamped (p < 0 -> 0), and a capped iterate of moving water is negative over large parts of the fluid: b - A p can only be formed
# on the cells `unclamped` keeps.  Every case is compared on those; the cases listed in CLAMP_FIT leave out less than CLAMP_CAP of the fluid cells (with the
# oracle alone: test_resident_ref_host.py) and assert that too.  Measured shares left out: random scenes 41 - 55 %, stirred grids 82 - 94 %, weird-edges
# 0.8 - 3.9 %, dam break 6.9 % (k = 1), 3.9 % (k = 5), 0.0 % (k = 40).  The 8 x 8 grid keeps no cell at all and is not part of this list.
RESIDUAL_CASES = [(n, k) for n in SCENES if n != "two_by_two_8x8" for k in caps(n, RESIDUAL_CAPS)]
CLAMP_FIT = [("weird_edges_257x129", 1), ("weird_edges_257x129", 5), ("weird_edges_257x129", 40), ("dam_break_65x300", 5), ("dam_break_65x300", 40)]


@functools.lru_cache(maxsize=None)
def scene_state(name):
    X, Y, text, upscale, frames, stir = SCENES[name]
    return moving_state(X, Y, text, frames, upscale=upscale, stir=stir)


@functools.lru_cache(maxsize=None)
def scene_capped(name, k, f32=False):
    return oracle_capped(scene_state(name), k, f32)
