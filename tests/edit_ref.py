"""The numpy restatement of euler_edit_box (include/euler.h, docs/editing.md) on a state dict - the dicts of resident_ref.moving_state / oracle_from_state and of
euler_amd.read_snapshot / write_snapshot - and the scenes the edit tests share (test_edit_host.py holds them to what the GPU tests need, with the oracle alone).

Deleting is the literal swap-with-last loop of refresh_marker_counts (main.c:105-116) with "the marker lies in the box" as its condition (delete_in_box, the
definition; edit_state uses delete_in_box_vectorised, the same array for millions of markers, which test_edit_host.py holds to the loop); seeding is
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


def delete_in_box_vectorised(markers, box):
    """delete_in_box restated for millions of markers: with D markers in the box and n' = n - D, the survivors below n' stay where they are and the k-th hole
    below n' (ascending) gets the k-th survivor at or above n', counted from the back.  test_edit_host.py holds it to the literal loop."""
    m = np.array(markers, np.float32).reshape(-1, 2)
    x0, y0, x1, y1 = box
    fx, fy = np.floor(m[:, 0]), np.floor(m[:, 1])
    gone = (x0 <= fx) & (fx <= x1) & (y0 <= fy) & (fy <= y1)
    n1 = len(m) - int(gone.sum())
    out = m[:n1].copy()
    out[np.nonzero(gone[:n1])[0]] = m[n1:][~gone[n1:]][::-1]
    return out


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
        st["markers"] = delete_in_box_vectorised(st["markers"], box)
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
    c = np.bincount(np.floor(m[:, 1]).astype(np.int64) * X + np.floor(m[:, 0]).astype(np.int64), minlength=X * Y).reshape(Y, X)
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


# ----------------------------------------------------------------------------- synthetic states and the structured boxes of test_gpu_edit_boxes.py
# 260 x 200 (X % 4 == 0: the interior is two census blocks wide, 5 x 4 workgroups of the cell pass) and 203 x 131 (ragged) hold boxes of more than one 64 x 64
# tile of the cell pass; the two small grids are the existing tests'.  grid -> (seed, n): odd and even marker counts.
BOX_GRIDS = {(96, 64): (11, 8741), (101, 45): (12, 6300), (260, 200): (13, 76383), (203, 131): (14, 38900)}
OP_NAMES = tuple(OPS)


@functools.lru_cache(maxsize=None)
def synthetic_state(X, Y, seed, n):
    """A seeded random state dict (the keys load_state of test_gpu_edit.py consumes), read-only: about 15 % solid, 3 % sink and 3 % source interior cells, mutually
    exclusive, the border as the loader leaves it (the upscaled dam break's); n float32 markers in non-solid interior cells (sink and source cells included), count =
    prev_count = their bins; small random u, v in the interior, zeros elsewhere.  Cell (1, 1) is open and empty, cell (X-2, Y-2) is open and holds marker 0: the
    two single-cell boxes are one eligible and one ineligible cell for FILL."""
    rng = np.random.default_rng(seed)
    st = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in base_state(X, Y, 0).items()}
    r = rng.random((Y - 2, X - 2))
    for name, lo, hi in (("solid", 0.0, 0.15), ("sink", 0.15, 0.18), ("source", 0.18, 0.21)):
        st[name][1:-1, 1:-1] = (lo <= r) & (r < hi)
        st[name][1, 1] = st[name][Y - 2, X - 2] = 0
    for name in ("u", "v"):
        st[name][...] = 0
        st[name][1:-1, 1:-1] = rng.uniform(-0.1, 0.1, (Y - 2, X - 2)).astype(np.float32)
    for name in ("utmp", "vtmp", "precon"):
        st[name][...] = 0
    open_ = st["solid"] == 0
    open_[0], open_[-1], open_[:, 0], open_[:, -1] = False, False, False, False
    open_[1, 1] = False
    ys, xs = np.nonzero(open_)
    pick = rng.integers(0, len(xs), n)
    cx, cy = xs[pick].astype(np.float32), ys[pick].astype(np.float32)
    if n:
        cx[0], cy[0] = X - 2, Y - 2
    # (a fraction in [0.001, 0.999]: the float32 sum stays inside the cell on every grid here)
    m = np.stack([cx + rng.uniform(0.001, 0.999, n).astype(np.float32), cy + rng.uniform(0.001, 0.999, n).astype(np.float32)], axis=1).astype(np.float32)
    assert np.array_equal(np.floor(m[:, 0]), cx) and np.array_equal(np.floor(m[:, 1]), cy)
    st["markers"] = m
    st["count"] = bins(m, X, Y)
    st["prev_count"] = st["count"].copy()
    st["rng_state"] = int(rng.integers(1, 1 << 63))
    st["source_exhausted"] = 0
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


def edge_markers(box):
    """eight float32 markers at the edges of the box: x exactly on x0, one ulp below it, exactly on x1 + 1, one ulp below it (y inside the box), and the same four
    in y (x inside) -> (the markers, whether each lies in the box)"""
    x0, y0, x1, y1 = box
    f, down = np.float32, lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    xs = [f(x0), down(x0), f(x1 + 1), down(x1 + 1)]
    ys = [f(y0), down(y0), f(y1 + 1), down(y1 + 1)]
    m = np.array([(x, f(y0 + 0.25)) for x in xs] + [(f(x0 + 0.75), y) for y in ys], np.float32)
    return m, np.array([True, False, False, True] * 2)


def with_edge_markers(state, box):
    """`state` with edge_markers(box) in its marker array: the four in x in front, the four in y behind (the grids are left as they are)"""
    e, _ = edge_markers(box)
    st = dict(state)
    st["markers"] = np.concatenate([e[:4], np.asarray(state["markers"], np.float32).reshape(-1, 2), e[4:]])
    return st


def box_families(X, Y):
    """-> {family: [(op name, box), ...]} for a grid of BOX_GRIDS.  A family of few boxes meets all six ops on every box; the ops of the others go round, starting
    at another op on each grid: every op meets every family on at least one grid (test_edit_host.py checks that, and the mix of cells and markers in each)."""
    g = list(BOX_GRIDS).index((X, Y))
    every = lambda boxes: [(op, b) for b in boxes for op in OP_NAMES]
    spread = lambda boxes: [(OP_NAMES[(g + i) % 6], b) for i, b in enumerate(boxes)]
    fam = {}
    if X % 4 == 0:      # the dword path: all 16 (x0 & 3, x1 & 3) with more than one column, and one column at each residue; heights 1 .. 5
        boxes = []
        for r0 in range(4):
            for r1 in range(4):
                i = 4 * r0 + r1
                x0 = 4 * (1 + (5 * i) % ((X - 24) // 4)) + r0
                boxes.append((x0, (x0 & ~3) + 4 * (1 + (r0 + r1) % 3) + r1))
        for r in range(4):
            x0 = 4 * (2 + 3 * r) + r
            boxes.append((x0, x0))
        fam["edge alignment"] = spread([(x0, 1 + (7 * i) % (Y - 7), x1, 1 + (7 * i) % (Y - 7) + i % 5) for i, (x0, x1) in enumerate(boxes)])
    fam["single cell"] = every([(1, 1, 1, 1), (X - 2, Y - 2, X - 2, Y - 2)])
    fam["whole interior"] = every([(1, 1, X - 2, Y - 2)])      # (the state: with_edge_markers - four of them lie in border cells, outside)
    if Y - 2 >= 65:      # columns of more than one 64-bit word of the mask, and of more than one workgroup
        boxes = []
        for h in sorted({65, 67, 128, 129, Y - 2}):
            for w in (1, 2, 3, 5):
                if h <= Y - 2:
                    i = len(boxes)
                    x0, y0 = 1 + (37 * i) % (X - 2 - w), 1 + (3 * i) % (Y - 1 - h)
                    boxes.append((x0, y0, x0 + w - 1, y0 + h - 1))
        fam["tall and narrow"] = spread(boxes)
    fam["wide and flat"] = every([(1, Y // 2 + 1, X - 2, Y // 2 + 1)])
    boxes = []
    for h in (66, 97, 131, 198):      # more than one workgroup each way: the 64-wide ones start at x0 & ~3 (X % 4 == 0) or x0, the 64-high ones at y0
        for w in (70, 101, 150):
            if h <= Y - 2 and w <= X - 2:
                i = len(boxes)
                x0, y0 = 1 + (13 * i + 2) % (X - 1 - w), 1 + (5 * i) % (Y - 1 - h)
                boxes.append((x0, y0, x0 + w - 1, y0 + h - 1))
    if boxes:
        fam["across workgroups"] = spread(boxes)
    fam["edge markers"] = every([(X // 3, Y // 3, X // 3 + 9, Y // 3 + 6)])      # (the state: with_edge_markers)
    for cases in fam.values():
        for _, (x0, y0, x1, y1) in cases:
            assert 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= Y - 2, (X, Y, x0, y0, x1, y1)
    return fam


def family_state(X, Y, family, box):
    """the state a case of box_families(X, Y) starts from"""
    st = synthetic_state(X, Y, *BOX_GRIDS[(X, Y)])
    return with_edge_markers(st, box) if family in ("edge markers", "whole interior") else st


def random_chain(X, Y, seed, length=12):
    """`length` seeded random (op name, box) pairs"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(length):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya, yb = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
        out.append((OP_NAMES[int(rng.integers(0, 6))], (xa, ya, xb, yb)))
    return out
