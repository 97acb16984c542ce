"""The numpy restatement of euler_edit_box (include/euler.h, docs/editing.md) on a state dict - the dicts of resident_ref.moving_state / oracle_from_state and of
euler_amd.read_snapshot / write_snapshot - and the scenes the edit tests share (test_edit_host.py holds them to what the GPU tests need, with the oracle alone).

Deleting is the literal swap-with-last loop of refresh_marker_counts (main.c:105-116) with "the marker lies in the box" as its condition; seeding is
euler_amd.seed_markers (sim_init's loop, main.c:255-266) over the eligible mask, from the state's RNG.

Test infrastructure only: nothing here touches the GPU."""
import functools

import numpy as np

import euler_amd as ea
from euler_amd import scenarios
from resident_ref import moving_state, oracle_from_state

OPS = {"solid": ea.EDIT_SOLID, "clear": ea.EDIT_CLEAR, "sink": ea.EDIT_SINK, "source": ea.EDIT_SOURCE, "fill": ea.EDIT_FILL, "drain": ea.EDIT_DRAIN}
GRID_NAMES = ("solid", "source", "sink", "count", "prev_count", "u", "v", "utmp", "vtmp", "precon")


class Refused(ValueError):
    """the edit would seed more markers than the array holds (EULER_EINVAL, the state unchanged)"""


def in_box(x, y, box):
    x0, y0, x1, y1 = box
    return x0 <= np.floor(x) <= x1 and y0 <= np.floor(y) <= y1


def delete_in_box(markers, box):
    """refresh_marker_counts' removal: the array walked in order, a deleted marker replaced by the current last one, which is examined next"""
    m = np.array(markers, np.float32).reshape(-1, 2)
    n, i = len(m), 0
    while i < n:
        if in_box(m[i, 0], m[i, 1], box):
            m[i] = m[n - 1]
            n -= 1
        else:
            i += 1
    return m[:n].copy()


def edit_state(state, op, box):
    """-> the edited copy of `state` (arrays writable); Refused when n + 4 E > 4 X Y - 1"""
    x0, y0, x1, y1 = box
    X, Y = state["u"].shape[1], state["u"].shape[0]
    assert 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= Y - 2 and op in OPS.values()
    st = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    if op in (ea.EDIT_SOLID, ea.EDIT_SINK, ea.EDIT_CLEAR, ea.EDIT_SOURCE):
        for name, one in (("solid", ea.EDIT_SOLID), ("sink", ea.EDIT_SINK), ("source", ea.EDIT_SOURCE)):
            st[name][sl] = 1 if op == one else 0
    if op in (ea.EDIT_SOLID, ea.EDIT_SINK, ea.EDIT_DRAIN):
        st["markers"] = delete_in_box(st["markers"], box)
        st["count"][sl] = 0
    if op in (ea.EDIT_SOURCE, ea.EDIT_FILL):
        elig = np.zeros((Y, X), np.uint8)
        elig[sl] = (st["solid"][sl] == 0) & (st["sink"][sl] == 0) & (st["count"][sl] == 0)
        if len(st["markers"]) + 4 * int(elig.sum()) > 4 * X * Y - 1:
            raise Refused("%d markers + 4 x %d cells" % (len(st["markers"]), int(elig.sum())))
        new, rng = ea.seed_markers(elig, int(st["rng_state"]))      # x outer, y inner; 8 draws per cell, the x draw first
        st["markers"] = np.concatenate([np.asarray(st["markers"], np.float32).reshape(-1, 2), new])
        st["rng_state"] = rng
        st["count"][elig != 0] = 4
    if "n_markers" in st:      # (a snapshot dict)
        st["n_markers"] = len(st["markers"])
    return st


def bins(markers, X, Y):
    """the marker counts per cell, as the uint8 grid the refresh would leave (it wraps)"""
    m = np.asarray(markers, np.float32).reshape(-1, 2)
    c = np.zeros((Y, X), np.int64)
    np.add.at(c, (np.floor(m[:, 1]).astype(np.int64), np.floor(m[:, 0]).astype(np.int64)), 1)
    return (c % 256).astype(np.uint8)


# ----------------------------------------------------------------------------- the scenes of the edit tests
# The upscaled dam break, edited after FRAMES_BEFORE frames and continued for FRAMES_AFTER: the block has hit the floor by then, so the frames after the edit have PCG
# iterations (with 10 frames after the edit most ops see none: the block is still in free fall).  The boxes are given on 96 x 64 and scaled to the other grids;
# 101 x 45 is ragged (X % 4 != 0), 130 x 70 has tile boundaries in x and y.
GRIDS = ((96, 64), (101, 45), (130, 70))
FRAMES_BEFORE, FRAMES_AFTER = 4, 25
BOXES_96x64 = {
    "solid": (40, 10, 45, 30),      # a wall through the falling block
    "fill": (70, 40, 85, 50),       # a block of water in the dry tile right of x = 64
    "drain": (10, 20, 20, 30),      # a hole in the block
    "clear": (1, 10, 1, 14),        # a notch in the left wall
    "sink": (30, 2, 35, 3),         # a drain in the floor
    "source": (5, 55, 8, 57),       # a tap under the ceiling
}
SEQUENCE = ("solid", "fill", "drain", "clear", "sink", "source")


# the upscaled picture's left wall is two cells thick on the two larger grids: the notch goes through both (a notch in the outer one alone opens nothing)
WIDER = {      # -> x1
    ("clear", 101, 45): 2, ("clear", 130, 70): 2,
}


def scaled_box(name, X, Y):
    x0, y0, x1, y1 = BOXES_96x64[name]
    sx0, sy0 = max(1, x0 * X // 96), max(1, y0 * Y // 64)
    sx1 = WIDER.get((name, X, Y), x1 * X // 96)
    return sx0, sy0, min(X - 2, max(sx0, sx1)), min(Y - 2, max(sy0, y1 * Y // 64))


@functools.lru_cache(maxsize=None)
def base_state(X, Y, frames=FRAMES_BEFORE, text=None):
    return moving_state(X, Y, text or scenarios.dam_break(), frames, upscale=True)


@functools.lru_cache(maxsize=None)
def edited_state(X, Y, what):
    """what: None (unedited), an op's name, or "sequence" (the six ops one after the other) -> the restated state, read-only"""
    st = base_state(X, Y)
    for name in () if what is None else SEQUENCE if what == "sequence" else (what,):
        st = edit_state(st, OPS[name], scaled_box(name, X, Y))
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


def parity_oracle(state):
    """the reference-identical oracle (IC(0), sequential sums) from a state"""
    o = oracle_from_state(state)
    o.c.tile_records = 0
    return o


FRAME_FIELDS = ("u", "v", "utmp", "vtmp", "count", "prev_count", "solid", "source", "sink")


@functools.lru_cache(maxsize=None)
def continued(X, Y, what, frames=FRAMES_AFTER):
    """The parity oracle stepped `frames` frames from edited_state(X, Y, what) -> a tuple of per-frame dicts: FRAME_FIELDS, markers (in order), rng_state, substeps,
    iterations.  Computed once and shared, read-only."""
    o = parity_oracle(edited_state(X, Y, what))
    out = []
    for _ in range(frames):
        sub, it = o.step()
        rec = {n: np.array(getattr(o, n)) for n in FRAME_FIELDS}
        rec["markers"] = np.array(o.markers)
        for v in rec.values():
            v.setflags(write=False)
        rec.update(rng_state=int(o.c.rng_state), substeps=int(sub), iterations=int(it), finite=bool(np.isfinite(o.u).all() and np.isfinite(o.v).all()))
        out.append(rec)
    o.close()
    return tuple(out)
