"""euler_gauges on the GPU (docs/gauges.md): the records of the batched device reduction against the numpy restatement (tests/gauges_ref.py) of the fields
read back through euler_get_field - every field exactly equal, the maxima bit for bit - over grids that take each path of the kernel, boxes that cut tiles,
bands and pair-records, random scenes with special values, the pressure of every solver mode, a known answer; that the pass leaves no trace in the state;
the five observer passes in turn; `euler --gauge / --gauges`."""
import subprocess

import numpy as np
import pytest

import diagnostics_ref as dref
import euler_amd as ea
import flow_ref as fref
import gauges_ref as gref
import overview_ref as ref
import viewport_ref as vref
from euler_amd import scenarios
from golden_util import X, Y, load, scenario_text
from observer_util import EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames, no_trace_pair
from test_gauges_host import hydrostatic_bound, random_boxes

pytestmark = pytest.mark.gpu

KINDS = (ea.GAUGE_LEVEL, ea.GAUGE_PRESSURE, ea.GAUGE_FORCE, ea.GAUGE_FLUX)
GRIDS = [(100, 40),      # one band
         (103, 41),      # odd width
         (264, 136),     # three bands, several tiles, dry tiles
         (1031, 70)]     # seventeen tile columns, two bands


def grids_of(sim):
    return [sim.get(f) for f in (ea.F_SOLID, ea.F_COUNT, ea.F_U, ea.F_V, ea.F_PRESSURE)]


def dry_tile_box(count):
    """a box strictly inside a 64 x 64 tile without a marker, None where every tile has some"""
    Yg, Xg = count.shape
    for ty in range((Yg + 63) // 64):
        for tx in range((Xg + 63) // 64):
            if not count[ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64].any():
                x0, y0, x1, y1 = max(tx * 64 + 3, 1), max(ty * 64 + 2, 1), min(tx * 64 + 40, Xg - 2), min(ty * 64 + 30, Yg - 2)
                if x0 <= x1 and y0 <= y1:
                    return (x0, y0, x1, y1)
    return None


def boxes_of(Xg, Yg, count=None, seed=0):
    """the whole interior, one cell, one row, one column, x0 odd and even (the parity of the pair-records), boxes across x = 63 | 64, y = 63 | 64 and
    y = 127 | 128 (clipped to the interior), boxes touching X - 2 and Y - 2, a box in a dry tile, 20 seeded random boxes, one box twice, two that overlap"""
    xi, yi = Xg - 2, Yg - 2
    clip = lambda b: (min(b[0], xi), min(b[1], yi), min(b[2], xi), min(b[3], yi))
    out = [(1, 1, xi, yi), (5, 6, 5, 6), (1, yi // 2, xi, yi // 2), (xi // 3, 1, xi // 3, yi),
           (3, 2, 20, 9), (4, 2, 21, 9), (7, 3, 7, 30), (8, 3, 8, 30),
           clip((60, 3, 70, 8)), clip((63, 1, 64, 12)), clip((64, 5, 127, 20)), clip((5, 60, 9, 70)), clip((2, 63, 40, 64)), clip((50, 120, 80, 133)), clip((61, 62, 66, 129)),
           (xi - 4, yi - 3, xi, yi), (xi, 1, xi, yi), (1, yi, xi, yi), (xi, yi, xi, yi), (1, 1, 1, 1)]
    if count is not None:
        dry = dry_tile_box(count)
        if dry:
            out.append(dry)
    out += random_boxes(np.random.default_rng(seed + Xg), Xg, Yg, 20)
    out += [out[4], (10, 4, 30, 12), (20, 8, 40, 16)]
    return out


def check(sim, gauges, what):
    """the device call comes FIRST, so that it is the one to finish a pending pressure; then every field of every record against the restatement"""
    got = sim.gauges(gauges)
    assert got.shape == (len(gauges),) and got.dtype == ea.GAUGE_REC_DTYPE
    g = grids_of(sim)
    bad = []
    for k, (kind, box) in enumerate(gauges):
        want = gref.gauge_ref(*g, kind, box)
        miss = gref.mismatches(got[k], want)
        if miss:
            bad.append((k, kind, box, miss, got[k], want))
    print("%s: %d gauges, %d records differ; fluid %d terms %d nonfinite %d" % (what, len(gauges), len(bad), int(got["fluid"].sum()), int(got["terms"].sum()), int(got["nonfinite"].sum())))
    assert not bad, (what, bad[:3])
    return got


def all_kinds(boxes):
    return [(kind, box) for box in boxes for kind in KINDS]


# ----------------------------------------------------------------------------- the surface
def test_refusals_in_order_and_the_buffer():
    sim = ea.Simulation(X, Y)
    L = sim.L
    sentinel = np.full(3, 0x5A, np.uint8).tobytes() * 24
    out = np.frombuffer(bytearray(sentinel * 4), ea.GAUGE_REC_DTYPE).copy()      # four records of 0x5a bytes
    untouched = out.tobytes()
    good = np.zeros(4, ea.GAUGE_DTYPE)
    for k in range(4):
        good[k] = (k, 2, 3, 20 + k, 9, 0)

    def call(s, g=good, n=None, o=out, nbytes=None):
        n = (4 if g is None else len(g)) if n is None else n
        return L.euler_gauges(s.h if s else None, g.ctypes.data if g is not None else None, n, o.ctypes.data if o is not None else None, 72 * n if nbytes is None else nbytes)

    assert call(None) == EULER_EINVAL and call(sim, g=None) == EULER_EINVAL and call(sim, o=None) == EULER_EINVAL      # a null argument comes first
    assert call(sim) == EULER_ESTATE                                    # nothing loaded
    wrong = good.copy()
    wrong["kind"][0] = 9
    assert call(sim, g=wrong, n=0, nbytes=1) == EULER_ESTATE             # ... in front of every other complaint
    before = sim.hbm_bytes()
    sim.load_text(scenario_text(load("basic_frames.npz")))
    for n in (0, -1, 1025, 1 << 20):
        assert call(sim, n=n, nbytes=72 * max(n, 0)) == EULER_EINVAL, n
    for nbytes in (0, 72 * 4 - 1, 72 * 5, 72, 24 * 4):
        assert call(sim, nbytes=nbytes) == EULER_EINVAL, nbytes
    assert call(sim, g=wrong, nbytes=5) == EULER_EINVAL and b"bytes" in L.euler_last_error()      # the byte count comes in front of the gauges
    for at in (0, 3):
        for field, val in (("kind", 4), ("kind", -1), ("reserved", 1), ("x0", 0), ("y0", 0), ("x1", X - 1), ("y1", Y - 1), ("x0", 30), ("y0", 12)):
            wrong = good.copy()
            wrong[field][at] = val
            assert call(sim, g=wrong) == EULER_EINVAL, (at, field, val)
            assert ("gauge %d " % at).encode() in L.euler_last_error(), L.euler_last_error()      # the message names the gauge
    wrong = good.copy()
    wrong["kind"][1], wrong["reserved"][0] = 7, 3
    assert call(sim, g=wrong) == EULER_EINVAL and b"gauge 0 " in L.euler_last_error()      # the first gauge refused is the one named
    assert sim.hbm_bytes() == before and out.tobytes() == untouched      # a refused call allocates nothing and leaves out untouched
    # the buffer: 72 bytes per record and 24 per chunk, grown on demand, kept, counted
    assert call(sim) == 0 and out.tobytes() != untouched
    assert sim.hbm_bytes() == before + 4 * (72 + 24)
    g = grids_of(sim)
    assert not gref.mismatches(out, gref.gauges_ref(*g, [(int(r["kind"]), (int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"]))) for r in good]))
    check(sim, [(ea.GAUGE_FORCE, (1, 1, X - 2, Y - 2))], "one gauge")      # n = 1: two tile columns, one tile row
    assert sim.hbm_bytes() == before + 4 * (72 + 24)
    many = [(k % 4, (1 + k % 98, 1 + k % 38, 1 + k % 98, 1 + k % 38)) for k in range(1024)]      # n = 1024 one-cell gauges
    recs = check(sim, many, "1024 one-cell gauges")
    assert (recs["cells"] == 1).all() and sim.hbm_bytes() == before + 1024 * (72 + 24)
    check(sim, all_kinds(boxes_of(X, Y)[:6]), "a shorter list in the kept buffer")
    assert sim.hbm_bytes() == before + 1024 * (72 + 24)
    with pytest.raises(ea.EulerError) as e:
        sim.gauges([(ea.GAUGE_LEVEL, (1, 1, X - 1, 5))])
    assert e.value.code == EULER_EINVAL and "gauge 0" in str(e.value)
    with pytest.raises(ea.EulerError) as e:
        sim.gauges([])
    assert e.value.code == EULER_EINVAL
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:
        slab.gauges([(ea.GAUGE_LEVEL, (1, 1, 5, 5))])
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    assert call(slab, g=wrong, n=0, nbytes=1) == EULER_ESTATE and out.tobytes() != untouched      # the slab refusal comes in front of the count and the gauges
    slab.close()


# ----------------------------------------------------------------------------- grids that exercise each path, in motion
@pytest.mark.parametrize("size", GRIDS)
def test_a_dam_break_in_motion_with_and_without_the_tile_map(size):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50).load_text(scenarios.dam_break(), upscale=True)
    for frame in (0, 6):
        while sim.stats().frames < frame:
            sim.step()
        count = sim.get(ea.F_COUNT)
        gauges = all_kinds(boxes_of(*size, count=count, seed=frame))
        if size == (264, 136):
            dry = dry_tile_box(count)
            assert dry is not None      # (the block leaves tiles of this grid without a marker)
            assert not count[dry[1]:dry[3] + 1, dry[0]:dry[2] + 1].any()
        sim.set_option(ea.OPT_NO_TILE_MAP, 0)
        a = check(sim, gauges, "%dx%d frame %d" % (size + (frame,)))
        sim.set_option(ea.OPT_NO_TILE_MAP, 1)
        b = check(sim, gauges, "%dx%d frame %d, no tile map" % (size + (frame,)))
        assert a.tobytes() == b.tobytes()
        whole = dict(zip(KINDS, a[:4]))
        assert whole[ea.GAUGE_LEVEL]["fluid"] > 0 and whole[ea.GAUGE_FLUX]["terms"] > 0
        if frame:
            assert whole[ea.GAUGE_FLUX]["b_neg"] > 0 and whole[ea.GAUGE_FLUX]["max_b"] > 0      # (the block is falling)
    sim.close()


# ----------------------------------------------------------------------------- random scenes through euler_set_field
def random_scene(sim, seed):
    rng = np.random.default_rng(seed)
    shape = (sim.Y, sim.X)
    solid = (rng.random(shape) < 0.15).astype(np.uint8)
    sink = (rng.random(shape) < 0.1).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.8, rng.choice(np.array([1, 2, 4, 8, 255], np.uint8), shape), 0).astype(np.uint8)
    u, v = (rng.standard_normal(shape).astype(np.float32) * 3 for _ in range(2))
    p = np.abs(rng.standard_normal(shape)) * 40.0
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5000.0, -4096.5, 1e30, -3e38, 4095.99], np.float32)
    for a, sp in ((u, special), (v, special), (p, np.array([np.nan, np.inf, -np.inf, -5.0, 1e30, 16777217.0, 3e-3, 0.0]))):
        hit = rng.random(shape) < 0.03
        a[hit] = rng.choice(sp, int(hit.sum()))
    for f, a in ((ea.F_SOLID, solid), (ea.F_SINK, sink), (ea.F_COUNT, count), (ea.F_U, u), (ea.F_V, v), (ea.F_PRESSURE, p)):
        sim.set(f, a)


@pytest.mark.parametrize("size", GRIDS)
def test_random_masks_with_planted_values(size):
    sim = ea.Simulation(*size).load_text(scenarios.dam_break(), upscale=True)
    for seed in (1, 2):
        random_scene(sim, seed + size[0])
        gauges = all_kinds(boxes_of(*size, seed=seed))
        sim.set_option(ea.OPT_NO_TILE_MAP, 0)
        a = check(sim, gauges, "%dx%d random %d" % (size + (seed,)))
        whole = dict(zip(KINDS, a[:4]))
        # (the planted values reach every kind: NaNs counted, infinities in the maxima, saturated terms in the sums)
        assert all(whole[k]["nonfinite"] > 0 for k in KINDS[1:]) and np.isinf(whole[ea.GAUGE_PRESSURE]["max_a"]) and np.isinf(whole[ea.GAUGE_FLUX]["max_a"])
        assert min(int(whole[ea.GAUGE_FLUX][n]) for n in ("a_pos", "a_neg", "b_pos", "b_neg")) > 4096 << 20 and whole[ea.GAUGE_PRESSURE]["a_pos"] > 1 << 32
        assert min(int(whole[ea.GAUGE_FORCE][n]) for n in ("a_pos", "a_neg", "b_pos", "b_neg")) > 0 and max(whole[ea.GAUGE_FORCE]["max_a"], whole[ea.GAUGE_FORCE]["max_b"]) >= 16777216
        sim.set_option(ea.OPT_NO_TILE_MAP, 1)
        assert check(sim, gauges, "%dx%d random %d, no tile map" % (size + (seed,))).tobytes() == a.tobytes()
    sim.close()


# ----------------------------------------------------------------------------- the pressure kinds
MODES = {"default": dict(dot_mode=ea.DOT_SEQUENTIAL),
         "tile-resident": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE),
         "tile-multikernel": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, resident=ea.RESIDENT_OFF),
         "tile-fp32": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, pcg_precision=ea.PCG_F32),
         "multilevel": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=400)}


@pytest.mark.parametrize("mode,size", [(m, (264, 136)) for m in sorted(MODES)] + [("default", (100, 40))])
def test_pressure_kinds_of_every_solver_mode(mode, size):
    sim = ea.Simulation(*size, **MODES[mode]).load_text(scenarios.dam_break(), upscale=True)
    boxes = boxes_of(*size)
    gauges = [(kind, box) for box in boxes for kind in (ea.GAUGE_PRESSURE, ea.GAUGE_FORCE)]
    fresh = check(sim, gauges, "%s %dx%d fresh" % ((mode,) + size))      # freshly loaded: the pressure is all 0
    assert not fresh["a_pos"].any() and not fresh["b_neg"].any() and not fresh["max_a"].any() and fresh["terms"].any()
    for _ in range(80):      # the block hangs above the floor: the solves begin when it lands
        sim.step()
        if sim.get(ea.F_PRESSURE).max() > 1.0:
            break
    sim.step()      # the pending pressure is finished by the gauges' own call, not by euler_get_field
    got = check(sim, gauges, "%s %dx%d solving" % ((mode,) + size))
    assert got[0]["a_pos"] > 0 and got[0]["max_a"] > 0 and got[1]["terms"] > 0 and sim.stats().total_pcg_iterations > 0      # the whole interior: pressure, and wetted walls
    sim.step()
    check(sim, [(ea.GAUGE_LEVEL, boxes[0]), (ea.GAUGE_FLUX, boxes[0])], "%s %dx%d kinds that leave the pressure alone" % ((mode,) + size))
    check(sim, gauges[:8], "%s %dx%d pending again" % ((mode,) + size))
    bw = size[0] // 4
    gate = (bw, 2, bw + 6, size[1] // 2)
    sim.edit_box(ea.EDIT_SOLID, gate)      # right behind an edit: water cells turned into a wall keep their stale pressure out of the records
    around = [(ea.GAUGE_FORCE, (gate[0] - 1, gate[1] - 1, gate[2] + 1, gate[3] + 1)), (ea.GAUGE_PRESSURE, gate), (ea.GAUGE_FLUX, (gate[0] - 1, 1, gate[0] - 1, size[1] - 2))]
    check(sim, gauges[:8] + around, "%s %dx%d after an edit" % ((mode,) + size))
    sim.step()
    check(sim, gauges[:8] + around, "%s %dx%d a frame after the edit" % ((mode,) + size))
    sim.close()


def test_hydrostatic_floor_force():
    """the half tank of the host test's known answer, one substep on the device: the same bound"""
    sim = ea.Simulation(64, 40, dot_mode=ea.DOT_SEQUENTIAL).load_half_tank()
    sim.substep(sim.timestep(0.1))
    rec = sim.gauges([(ea.GAUGE_FORCE, (1, 1, 62, 38))])[0]
    assert sim.stats().last_pcg_iterations < 100
    d = hydrostatic_bound(rec)
    assert d["b"] == -10800.0 and rec["fluid"] == 1080
    assert not gref.mismatches(rec, gref.gauge_ref(*grids_of(sim), gref.FORCE, (1, 1, 62, 38)))
    lo = int(rec["lo_x"])      # (the extent of the water: its first column stands against the left wall)
    side = sim.gauges([(ea.GAUGE_FORCE, (lo, 1, lo, 38))])[0]      # the 18 cells along the left wall: 10 (1 + ... + 18) on it, towards -x
    assert side["a_pos"] == 0 and side["b_pos"] == 0 and side["fluid"] == 18
    assert abs(ea.gauge_derive(side, ea.GAUGE_FORCE)["a"] + 1710.0) <= 1e-4 * 1710.0
    sim.close()


# ----------------------------------------------------------------------------- no lasting state
def _pair(options=(), **kw):
    mixed = all_kinds([(1, 1, 254, 254), (100, 3, 100, 200), (60, 60, 70, 130), (3, 3, 3, 3)])

    def make():
        s = ea.Simulation(256, 256, max_iterations=40, **kw)
        for k, v in options:
            s.set_option(k, v)
        return s.load_text(scenarios.dam_break(), upscale=True)

    def look(s, stepped):
        s.gauges(mixed if stepped else mixed[:6])
        s.gauges([(ea.GAUGE_FLUX, (128, 1, 128, 254))] if stepped else [(ea.GAUGE_FORCE, (1, 1, 254, 5))])

    for s in no_trace_pair(make, look, None, STATE_FIELDS, 20, compare_every=5):
        s.close()


def test_the_pass_leaves_no_trace():
    _pair(dot_mode=ea.DOT_SEQUENTIAL)


def test_no_trace_with_maccormack_and_rk2():
    _pair(options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)), dot_mode=ea.DOT_SEQUENTIAL)


def test_no_trace_with_viscosity():
    _pair(dot_mode=ea.DOT_SEQUENTIAL, viscosity=0.5)


def test_no_trace_with_the_tile_solver():
    _pair(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE)


# ----------------------------------------------------------------------------- the five observer passes in turn
@pytest.mark.parametrize("size", [(70, 45), (72, 45)])
def test_the_five_passes_take_turns_on_one_handle(size):
    Xg, Yg = size
    sim = ea.Simulation(Xg, Yg, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True).load_text(scenario_text(load("block_frames.npz")), upscale=True)
    for _ in range(5):
        sim.step()
    p = sim.get(ea.F_PRESSURE)
    g = [sim.get(f) for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT, ea.F_U, ea.F_V)]
    dye = tuple(sim.get(f) for f in (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B))
    markers = sim.get(ea.F_MARKERS)
    dterms, fterms = dref.cell_terms(g[0], g[2], g[3], g[4]), fref.cell_terms(*g, p=p)
    rounds = []
    for order in ((0, 1, 2, 3, 4), (4, 3, 1, 0, 2), (2, 4, 0, 3, 1)):
        out = [None] * 5
        for box in ((35, 20, 35, 20), (1, 1, Xg - 2, Yg - 2), (57, 7, 66, 30)):
            bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
            w, h = max(1, bw // 3), max(1, bh // 2)
            for k in order:
                if k == 0:
                    got = sim.diagnostics_record(box)
                    assert not dref.mismatches(got, dref.reduce_box(dterms, box)), box
                elif k == 1:
                    got = sim.overview(w, h, box=box)
                    assert not ref.mismatches(got, vref.overview_box_ref(*g, dye, box, w, h)), box
                elif k == 2:
                    got = sim.marker_raster(box, 2)
                    assert np.array_equal(got, vref.raster_ref(markers, box, 2)), box
                elif k == 3:
                    got = sim.flow(w, h, box=box, pressure=True)
                    assert not fref.mismatches(got, fref.reduce_box(fterms, box, w, h)), box
                else:
                    got = sim.gauges(all_kinds([box, (1, 1, 5, 5)]))
                    assert not gref.mismatches(got, gref.gauges_ref(g[0], g[2], g[3], g[4], p, all_kinds([box, (1, 1, 5, 5)]))), box
                out[k] = (out[k] or b"") + got.tobytes()
        rounds.append(out)
    assert rounds[0] == rounds[1] == rounds[2]
    sim.close()


# ----------------------------------------------------------------------------- the front end
GATE = (60, 2, 62, 20)      # right of the block: the collapsing water runs against it
CLI_GAUGES = [(ea.GAUGE_FORCE, (GATE[0] - 1, GATE[1] - 1, GATE[2] + 1, GATE[3] + 1)),      # the load on the gate: its box grown by one cell
              (ea.GAUGE_FLUX, (61, 1, 61, 38)),                                             # the discharge through the gate's section
              (ea.GAUGE_LEVEL, (1, 1, 98, 38)), (ea.GAUGE_PRESSURE, (30, 3, 30, 3)), (ea.GAUGE_LEVEL, (20, 1, 24, 38))]


def _gauge_flags(gauges=CLI_GAUGES):
    out = []
    for kind, box in gauges:
        out += ["--gauge", "%s:%d,%d,%d,%d" % ((gref.KINDS[kind],) + tuple(box))]
    return out


def _python_csv(text, frames, every=1, edit_frame=10):
    sim = ea.Simulation(X, Y).load_text(text)
    out = [gref.CSV_HEADER]
    seen = np.zeros(0, ea.GAUGE_REC_DTYPE)
    for f in range(frames + 1):
        if f:
            if f == edit_frame:
                sim.edit_box(ea.EDIT_SOLID, GATE)
            sim.step()
        if f % every == 0:
            recs = sim.gauges(CLI_GAUGES)
            assert not gref.mismatches(recs, gref.gauges_ref(*grids_of(sim), CLI_GAUGES)), f
            out += [gref.csv_line(f, k, kind, recs[k]) for k, (kind, _) in enumerate(CLI_GAUGES)]
            seen = np.concatenate([seen, recs])
    sim.close()
    return "".join(out), seen


def test_cli_gauges(tmp_path):
    text = scenario_text(load("block_frames.npz"))
    scn = tmp_path / "block.txt"
    scn.write_text(text)
    edit = ["--edit", "10:solid:%d,%d,%d,%d" % GATE]
    base = [EXE, "--dump", "--window", "49x19"]

    def run(*flags, frames=60):
        r = subprocess.run(base + ["--frames", str(frames)] + list(flags) + [str(scn)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    # 60 frames with a gate closed at frame 10: the file is what Python writes from Simulation.gauges, line for line
    want, seen = _python_csv(text, 60)
    out = tmp_path / "g.csv"
    frames_with = run(*edit, *_gauge_flags(), "--gauges", str(out))
    assert out.read_text() == want
    print("the gate: wetted faces %d ... %d, largest face pressure %g" % (int(seen["terms"][0::5].min()), int(seen["terms"][0::5].max()), float(seen["max_a"][0::5].max())))
    assert seen["terms"][0::5].max() > 0 and seen["fluid"][2::5].min() > 0 and len(set(want.splitlines())) > 5 * 30      # (the scene moves: the lines differ from frame to frame)
    # the frames are those of a run without the flags
    assert frames_with == run(*edit)
    # --gauges-every, and the file truncated
    want7, _ = _python_csv(text, 30, every=7)
    run(*edit, *_gauge_flags(), "--gauges", str(out), "--gauges-every", "7", frames=30)
    assert out.read_text() == want7 and want7.count("\n") == 1 + 5 * 5
    # together with --stats, --fit and --ppm: the same file, and their outputs what they are without the gauges
    want12, _ = _python_csv(text, 12)
    plain_stats, both_stats = tmp_path / "s0.csv", tmp_path / "s1.csv"
    a = run(*edit, "--fit", "--stats", str(plain_stats), "--ppm", str(tmp_path / "a_"), "--ppm-size", "40x16", frames=12)
    b = run(*edit, "--fit", "--stats", str(both_stats), "--ppm", str(tmp_path / "b_"), "--ppm-size", "40x16", *_gauge_flags(), "--gauges", str(out), frames=12)
    assert out.read_text() == want12 and a == b and plain_stats.read_bytes() == both_stats.read_bytes()
    for f in (0, 12):
        assert (tmp_path / ("a_%06d.ppm" % f)).read_bytes() == (tmp_path / ("b_%06d.ppm" % f)).read_bytes()
    # a run without the flags is byte for byte what it was: the frames of euler_render
    sim = ea.Simulation(X, Y).load_text(text)
    plain = []
    for f in range(4):
        if f:
            sim.step()
        plain.append(sim.draw(49, 19))
    sim.close()
    assert dumped_frames(run(frames=3)) == plain
    # usage errors, status 1, nothing on stdout
    many = []
    for k in range(65):
        many += ["--gauge", "level:1,1,%d,5" % (k + 1)]
    for bad in (_gauge_flags(), ["--gauges", str(out)], ["--gauges", str(out), "--gauge", "heat:1,1,5,5"], ["--gauges", str(out), "--gauge", "level:1,1,5"],
                ["--gauges", str(out), "--gauge", "level:1,1,5,5x"], ["--gauges", str(out), "--gauge", "level"], ["--gauges", str(out), "--gauge", "flux:0,1,5,5"],
                ["--gauges", str(out), "--gauge", "flux:1,1,%d,5" % (X - 1)], ["--gauges", str(out), "--gauge", "flux:6,1,5,5"], ["--gauges", str(out)] + many,
                ["--gauges", str(out), "--gauges-every", "0"] + _gauge_flags()):
        r = subprocess.run(base + ["--frames", "2"] + bad + [str(scn)], capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--gauges FILE" in r.stderr and not r.stdout, bad
    r = subprocess.run(base + ["--frames", "2", "--gauges", str(out)] + many[:128] + [str(scn)], capture_output=True, timeout=60)      # 64 are taken
    assert r.returncode == 0 and out.read_text().count("\n") == 1 + 64 * 3
    # a write error ends the run with status 1
    r = subprocess.run(base + ["--frames", "2", "--gauges", str(tmp_path / "no_such_dir" / "g.csv")] + _gauge_flags() + [str(scn)], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"cannot write" in r.stderr
