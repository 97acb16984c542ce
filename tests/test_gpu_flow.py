"""euler_flow_raster on the GPU (docs/flow_raster.md): the records of the device reduction against the numpy restatement (tests/flow_ref.py) of the
fields read back through euler_get_field - every field exactly equal, the maxima bit for bit - over grids that take each path of the kernel, boxes that
cut a lane's group or touch the interior's edges, rasters from one pixel to one cell per pixel, random scenes with special values, a known answer, the
pressure of every solver mode; that the pass leaves no trace in the state; the four observer passes in turn; `euler --paint`."""
import subprocess

import numpy as np
import pytest

import diagnostics_ref as dref
import euler_amd as ea
import flow_ref as fref
import overview_ref as ref
import viewport_ref as vref
from euler_amd import scenarios
from golden_util import X, Y, load, scenario_text
from observer_util import EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames, no_trace_pair
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

GRIDS = [(100, 40),      # four cells per lane
         (103, 41),      # one per lane
         (264, 136),     # several tile rows and columns, dry tiles, three bands of the skewed pressure
         (1096, 72),     # more than one workgroup along a row, four cells per lane
         (1031, 70)]     # ... one per lane


def grids_of(sim):
    return [sim.get(f) for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT, ea.F_U, ea.F_V)]


def cases(Xg, Yg):
    """(box, w, h): the whole interior at 1 x 1 (tall boxes: split into row slices), one cell per pixel and 7 x 5; x0 % 4 = 3 and x0 % 4 = 2 cut a lane group;
    boxes that touch x1 = X - 2 and y1 = Y - 2; one cell; a box inside the first tile"""
    whole = (1, 1, Xg - 2, Yg - 2)
    out = [(whole, 1, 1), (whole, Xg - 2, Yg - 2), (whole, 7, 5)]
    cut = (3, 2, Xg - 4, Yg - 3)
    out += [(cut, 7, 5), (cut, cut[2] - cut[0] + 1, cut[3] - cut[1] + 1), (cut, 1, 1)]
    edge = (Xg // 2 + 2, Yg // 2, Xg - 2, Yg - 2)
    out += [(edge, 5, 3), (edge, edge[2] - edge[0] + 1, 1), (edge, 1, edge[3] - edge[1] + 1)]
    out += [((Xg - 2, Yg - 2, Xg - 2, Yg - 2), 1, 1), ((5, 6, 5, 6), 1, 1), ((2, 3, 30, 20), 29, 18), ((2, 3, 30, 20), 4, 4)]
    return out


def check(sim, what, pressure=False, which=None, terms=None):
    """every case of the handle's grid; with the pressure the device call comes FIRST, so that it is the one to finish the pending pressure"""
    todo = which or cases(sim.X, sim.Y)
    got = [sim.flow(w, h, box=box, pressure=pressure) for (box, w, h) in todo]
    terms = terms or fref.cell_terms(*grids_of(sim), p=sim.get(ea.F_PRESSURE) if pressure else None)
    for (box, w, h), g in zip(todo, got):
        assert g.shape == (h, w) and g.dtype == ea.FLOW_DTYPE
        want = fref.reduce_box(terms, box, w, h)
        bad = fref.mismatches(g, want)
        if bad or (w, h) == (1, 1):
            print("%s box %s %dx%d: water %d nodes %d nonfinite %d p_sum %d max |w| %g; fields that differ: %s" %
                  (what, box, w, h, int(want["water"].sum()), int(want["nodes"].sum()), int(want["nonfinite"].sum()), int(want["p_sum"].sum()), float(want["max_abs_w"].max()), bad or "none"))
        assert not bad, (what, box, w, h, bad)
        if not pressure:
            assert not g["p_sum"].any() and not g["max_p"].any()
        assert not g["reserved"].any()
    return terms


# ----------------------------------------------------------------------------- the surface
def test_refusals_in_order_and_the_buffer():
    sim = ea.Simulation(X, Y)
    L, buf = sim.L, np.zeros(50, ea.FLOW_DTYPE)
    call = lambda s, box=(1, 1, 20, 10), w=10, h=5, flags=0, out=buf, nbytes=88 * 50: L.euler_flow_raster(s.h if s else None, *box, w, h, flags, out.ctypes.data if out is not None else None, nbytes)
    assert call(None) == EULER_EINVAL and call(sim, out=None) == EULER_EINVAL      # a null argument comes first
    assert call(sim) == EULER_ESTATE                                                # nothing loaded
    assert call(sim, box=(0, 0, 500, 500), w=0, nbytes=1, flags=8) == EULER_ESTATE   # ... in front of every other complaint
    before = sim.hbm_bytes()
    sim.load_text(scenario_text(load("basic_frames.npz")))
    for box in ((0, 1, 5, 5), (1, 0, 5, 5), (1, 1, X - 1, 5), (1, 1, 5, Y - 1), (6, 1, 5, 5), (1, 6, 5, 5)):
        assert call(sim, box=box, w=1, h=1, nbytes=88) == EULER_EINVAL, box
    for (w, h) in ((0, 5), (5, 0), (-1, 5), (21, 5), (10, 11)):
        assert call(sim, w=w, h=h, nbytes=88 * max(w, 0) * max(h, 0)) == EULER_EINVAL, (w, h)
    for nbytes in (0, 88 * 50 - 1, 88 * 51, 88):
        assert call(sim, nbytes=nbytes) == EULER_EINVAL, nbytes
    for flags in (2, 3, -1, 1 << 20):
        assert call(sim, flags=flags) == EULER_EINVAL, flags
    assert sim.hbm_bytes() == before                      # a refused call allocates nothing
    assert call(sim) == 0 and call(sim, flags=ea.FLOW_PRESSURE) == 0
    assert sim.hbm_bytes() == before + 88 * 50
    terms = fref.cell_terms(*grids_of(sim))
    whole = (1, 1, X - 2, Y - 2)
    for (w, h) in ((3, 2), (98, 38), (7, 5), (98, 38), (1, 1)):      # the buffer grows and is kept
        assert not fref.mismatches(sim.flow(w, h), fref.reduce_box(terms, whole, w, h)), (w, h)
    assert sim.hbm_bytes() == before + 88 * 98 * 38
    with pytest.raises(ea.EulerError) as e:
        sim.flow(10, 5, box=(1, 1, 5, 5))
    assert e.value.code == EULER_EINVAL
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:
        slab.flow(10, 10)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    assert call(slab, box=(0, 0, 500, 500), w=0, nbytes=1, flags=8) == EULER_ESTATE      # the slab refusal comes in front of the box and the raster
    slab.close()


# ----------------------------------------------------------------------------- grids that exercise each path, in motion
@pytest.mark.parametrize("size", GRIDS)
def test_a_dam_break_in_motion_with_and_without_the_tile_map(size):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50).load_text(scenarios.dam_break(), upscale=True)
    check(sim, "%dx%d frame 0" % size)
    for _ in range(6):
        sim.step()
    t = check(sim, "%dx%d" % size)
    whole = fref.reduce_box(t, (1, 1, size[0] - 2, size[1] - 2), 1, 1)
    assert whole["water"] > 0 and whole["nodes"] > 0 and whole["max_speed2"] > 0 and whole["v_neg"] > 0      # (the column is falling; it has not begun to turn)
    sim.set_option(ea.OPT_NO_TILE_MAP, 1)
    check(sim, "%dx%d, no tile map" % size, terms=t)
    sim.close()


# ----------------------------------------------------------------------------- random scenes through euler_set_field
def random_scene(sim, seed):
    rng = np.random.default_rng(seed)
    shape = (sim.Y, sim.X)
    solid = (rng.random(shape) < 0.1).astype(np.uint8)
    sink = (rng.random(shape) < 0.1).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.85, rng.choice(np.array([1, 2, 4, 8, 255], np.uint8), shape), 0).astype(np.uint8)
    u, v = (rng.standard_normal(shape).astype(np.float32) * 3 for _ in range(2))
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5000.0, -4096.5, 1e30, -3e38, 4095.99], np.float32)
    for a in (u, v):
        hit = rng.random(shape) < 0.03
        a[hit] = rng.choice(special, int(hit.sum()))
    for f, a in ((ea.F_SOLID, solid), (ea.F_SINK, sink), (ea.F_COUNT, count), (ea.F_U, u), (ea.F_V, v)):
        sim.set(f, a)


@pytest.mark.parametrize("size", GRIDS)
def test_random_scenes_with_special_values(size):
    sim = ea.Simulation(*size).load_text(scenarios.dam_break(), upscale=True)
    for seed in (1, 2):
        random_scene(sim, seed + size[0])
        sim.set_option(ea.OPT_NO_TILE_MAP, 0)
        t = check(sim, "%dx%d random %d" % (size + (seed,)))
        whole = fref.reduce_box(t, (1, 1, size[0] - 2, size[1] - 2), 1, 1)
        assert whole["nonfinite"] > 0 and whole["nodes"] > 0 and np.isinf(whole["max_speed2"]) and np.isinf(whole["max_abs_w"])
        assert min(int(whole[n][0, 0]) for n in ("u_pos", "u_neg", "v_pos", "v_neg", "w_pos", "w_neg")) > 4096 << 20      # (saturated terms among them)
        sim.set_option(ea.OPT_NO_TILE_MAP, 1)
        check(sim, "%dx%d random %d, no tile map" % (size + (seed,)), terms=t)
    sim.close()


# ----------------------------------------------------------------------------- a known answer: solid-body rotation
@pytest.mark.parametrize("size", [(100, 40), (103, 41)])
def test_solid_body_rotation_has_vorticity_one(size):
    Xg, Yg = size
    sim = ea.Simulation(Xg, Yg).load_text("\n".join(["0" * 8] * 8), upscale=True)      # all water
    yy, xx = np.mgrid[0:Yg, 0:Xg].astype(np.float32)
    xc, yc = np.float32(Xg // 2), np.float32(Yg // 2)
    sim.set(ea.F_U, np.float32(-0.5) * (yy + np.float32(0.5) - yc))      # exact in float32
    sim.set(ea.F_V, np.float32(0.5) * (xx + np.float32(0.5) - xc))
    t = check(sim, "%dx%d rotation" % size)
    for (box, w, h) in cases(Xg, Yg):
        g = sim.flow(w, h, box=box)
        assert np.array_equal(g["water"], g["cells"])
        assert np.array_equal(g["w_pos"], g["nodes"].astype(np.uint64) << np.uint64(20)) and not g["w_neg"].any() and not g["nonfinite"].any()
        assert (g["max_abs_w"][g["nodes"] > 0] == np.float32(1)).all() and (g["max_abs_w"][g["nodes"] == 0] == 0).all()
    assert int(sim.flow(1, 1)["nodes"][0, 0]) == (Xg - 3) * (Yg - 3)      # every interior node but those against the sink ring
    sim.close()


# ----------------------------------------------------------------------------- the pressure
MODES = {"default": dict(dot_mode=ea.DOT_SEQUENTIAL),
         "tile-resident": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE),
         "tile-multikernel": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, resident=ea.RESIDENT_OFF),
         "tile-fp32": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, pcg_precision=ea.PCG_F32),
         "multilevel": dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=400)}


@pytest.mark.parametrize("size", [(100, 40), (264, 136)])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_pressure_of_every_solver_mode(mode, size):
    sim = ea.Simulation(*size, **MODES[mode]).load_text(scenarios.dam_break(), upscale=True)
    t = check(sim, "%s %dx%d fresh" % ((mode,) + size), pressure=True)      # freshly loaded: the pressure is all 0
    assert not t["p_sum"].any() and not t["max_p"].any()
    for _ in range(80):      # the block hangs above the floor: the solves begin when it lands, and a pressure below 2^-8 still sums to 0
        sim.step()
        if sim.get(ea.F_PRESSURE).max() > 1.0:
            break
    sim.step()
    t = check(sim, "%s %dx%d" % ((mode,) + size), pressure=True)
    whole = fref.reduce_box(t, (1, 1, size[0] - 2, size[1] - 2), 1, 1)
    assert whole["p_sum"] > 0 and whole["max_p"] > 0 and sim.stats().total_pcg_iterations > 0
    check(sim, "%s %dx%d without the flag" % ((mode,) + size), which=cases(*size)[:3])
    sim.step()      # the pending pressure finished by the raster's own call, not by euler_get_field
    got = sim.flow(7, 5, pressure=True)
    assert not fref.mismatches(got, fref.flow_ref(*grids_of(sim), (1, 1, size[0] - 2, size[1] - 2), 7, 5, p=sim.get(ea.F_PRESSURE)))
    bw = size[0] // 4
    sim.edit_box(ea.EDIT_SOLID, (bw, 2, bw + 6, size[1] // 2))      # right behind an edit: water cells turned into a wall keep their stale pressure out of the record
    check(sim, "%s %dx%d after an edit" % ((mode,) + size), pressure=True, which=cases(*size)[:4])
    sim.step()
    check(sim, "%s %dx%d a frame after the edit" % ((mode,) + size), pressure=True, which=cases(*size)[:4])
    sim.close()


def test_planted_pressures():
    """NaN, infinities, negative and huge values in the pressure (euler_set_field): a NaN counts its cell once, also where its velocity is a NaN too"""
    sim = ea.Simulation(264, 136, dot_mode=ea.DOT_TREE).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(3):
        sim.step()
    p, u = sim.get(ea.F_PRESSURE), sim.get(ea.F_U)
    wet = np.argwhere((sim.get(ea.F_COUNT) > 0) & (sim.get(ea.F_SOLID) == 0) & (sim.get(ea.F_SINK) == 0))
    assert len(wet) > 200
    for k, (y, x) in enumerate(wet[:: len(wet) // 60]):
        p[y, x] = (np.nan, np.inf, -np.inf, -5.0, 1e30, 16777217.0, 3e-3, np.nan)[k % 8]
        if k % 8 == 7:
            u[y, x] = np.nan
    sim.set(ea.F_PRESSURE, p); sim.set(ea.F_U, u)
    t = check(sim, "planted pressures", pressure=True)
    whole = fref.reduce_box(t, (1, 1, 262, 134), 1, 1)
    assert whole["nonfinite"] >= 15 and np.isinf(whole["max_p"])
    sim.close()


# ----------------------------------------------------------------------------- no lasting state
def _pair(scn, frames=12, options=(), **kw):
    text = scenario_text(load(scn + "_frames.npz"))

    def make():
        s = ea.Simulation(X, Y, **kw).load_text(text)
        for k, v in options:
            s.set_option(k, v)
        return s

    def look(s, stepped):
        s.flow(98, 38, pressure=stepped)
        s.flow(7, 5, box=(3, 2, 60, 30), pressure=not stepped)

    for s in no_trace_pair(make, look, None, STATE_FIELDS, frames):
        s.close()


def test_the_pass_leaves_no_trace():
    _pair("basic", dot_mode=ea.DOT_SEQUENTIAL)


def test_no_trace_with_the_tile_solver():
    _pair("block", dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE)


def test_no_trace_with_maccormack():
    _pair("filter", options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)), dot_mode=ea.DOT_SEQUENTIAL)


def test_no_trace_with_viscosity():
    _pair("waterfall", dot_mode=ea.DOT_SEQUENTIAL, viscosity=0.5)


def test_no_trace_on_a_lean_grid():
    """the grid passes in their lean forms (tile map, four cells per thread from 2^20 cells on here), whose validity flags the pass must not touch"""
    kw = dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=30)
    a, b = (ea.Simulation(1024, 1024, **kw).set_option(ea.OPT_GRID4_MIN_CELLS, 1 << 20).load_text(scenarios.dam_break(), upscale=True) for _ in range(2))
    for f in range(6):
        b.flow(200, 50, pressure=bool(f % 2))
        a.step(); b.step()
        b.flow(1022, 1022, pressure=not f % 2)
    for fld in (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP, ea.F_COUNT, ea.F_MARKERS, ea.F_PRESSURE):
        assert_bits(b.get(fld), a.get(fld), "field %d" % fld)
    a.close(); b.close()


# ----------------------------------------------------------------------------- the four observer passes in turn
@pytest.mark.parametrize("size", [(70, 45), (72, 45)])
def test_the_four_passes_take_turns_on_one_handle(size):
    Xg, Yg = size
    sim = ea.Simulation(Xg, Yg, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True).load_text(scenario_text(load("block_frames.npz")), upscale=True)
    for _ in range(5):
        sim.step()
    p = sim.get(ea.F_PRESSURE)
    g = grids_of(sim)
    dye = tuple(sim.get(f) for f in (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B))
    markers = sim.get(ea.F_MARKERS)
    dterms, fterms = dref.cell_terms(g[0], g[2], g[3], g[4]), fref.cell_terms(*g, p=p)
    rounds = []
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (0, 1, 2, 3)):
        out = [None] * 4
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
                else:
                    got = sim.flow(w, h, box=box, pressure=True)
                    assert not fref.mismatches(got, fref.reduce_box(fterms, box, w, h)), box
                out[k] = (out[k] or b"") + got.tobytes()
        rounds.append(out)
    assert rounds[0] == rounds[1] == rounds[2]
    sim.close()


# ----------------------------------------------------------------------------- the front end
def _composition(sim, box, view, wx, wy, field, scale):
    """what `euler --paint` draws: the records of euler_render_fit / euler_render_view, painted"""
    bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
    s = vref.view_zoom(bw, bh, wx, wy) if view else 0
    w, h = (bw, bh) if s else (min(wx, bw), min(wy, bh))
    px = ea.flow_paint(sim.flow(w, h, box=box, pressure=field == ea.PAINT_PRESSURE), sim.overview(w, h, box=box), field, scale)
    return ea.view_text(px, sim.marker_raster(box, s), s, rainbow=True) if s else ea.overview_text(px, rainbow=True)


def test_cli_paint(tmp_path):
    g = load("basic_frames.npz")
    scn = tmp_path / "basic.txt"
    scn.write_text(scenario_text(g))
    whole, small, tiny = (1, 1, X - 2, Y - 2), (10, 5, 80, 30), (40, 3, 51, 10)      # tiny: 12 x 8 cells in a 49 x 19 window: the markers' raster at scale 2
    assert vref.view_zoom(12, 8, 49, 19) == 2 and vref.view_zoom(71, 26, 49, 19) == 0
    sim = ea.Simulation(X, Y).load_text(scenario_text(g))
    want = {k: [] for k in ("fit", "view", "zoom", "plain_fit", "plain_view")}
    images = {}
    for f in range(4):
        if f:
            sim.step()
        want["fit"].append(_composition(sim, whole, False, 49, 19, ea.PAINT_VORTICITY, 2.0))
        want["view"].append(_composition(sim, small, True, 49, 19, ea.PAINT_PRESSURE, 30.0))
        want["zoom"].append(_composition(sim, tiny, True, 49, 19, ea.PAINT_SPEED, 4.0))
        want["plain_fit"].append(sim.render_fit(49, 19))
        want["plain_view"].append(sim.render_view(small, 49, 19))
        images[f] = ea.overview_rgb(ea.flow_paint(sim.flow(40, 16), sim.overview(40, 16), ea.PAINT_VORTICITY, 2.0), ea.IMAGE_DYE)
    sim.close()
    base = [EXE, "--dump", "--window", "49x19", "--frames", "3"]
    view = ["--view", "%d,%d,%d,%d" % small]

    def frames(*flags):
        run = subprocess.run(base + list(flags) + [str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0, run.stderr.decode()
        return dumped_frames(run.stdout)

    assert frames("--fit", "--paint", "vorticity:2") == want["fit"]
    assert frames(*view, "--paint", "pressure:30") == want["view"]
    assert frames("--view", "%d,%d,%d,%d" % tiny, "--paint", "speed:4") == want["zoom"]
    # without --paint and without v every byte is what it was
    assert frames("--fit") == want["plain_fit"] and frames(*view) == want["plain_view"] and frames(*view, "--keys", "h.l")[0] == want["plain_view"][0]
    assert want["fit"] != want["plain_fit"]
    # --ppm: the painted records in the dye mode, whatever --ppm-mode says; the dumped frames are the unpainted corner of draw
    prefix = str(tmp_path / "img_")
    plain = frames()
    assert frames("--ppm", prefix, "--ppm-size", "40x16", "--ppm-mode", "coverage", "--paint", "vorticity:2") == plain
    for f, rgb in images.items():
        wantp = tmp_path / "want.ppm"
        ea.write_ppm(str(wantp), rgb)
        assert (tmp_path / ("img_%06d.ppm" % f)).read_bytes() == wantp.read_bytes(), f
    # usage errors, status 1
    for bad in (["--paint", "vorticity:2"], ["--fit", "--paint", "heat:1"], ["--fit", "--paint", "speed:0"], ["--fit", "--paint", "speed:-1"], ["--fit", "--paint", "pressure:1x"],
                ["--fit", "--paint", "vorticity"], ["--fit", "--paint", "pressure:nan"], ["--fit", "--paint", "speed:inf"]):
        run = subprocess.run(base + bad + [str(scn)], capture_output=True, timeout=60)
        assert run.returncode == 1 and b"--paint vorticity:S" in run.stderr and not run.stdout, bad


def test_cli_v_key_cycles_the_fields(tmp_path):
    g = load("block_frames.npz")
    scn = tmp_path / "block.txt"
    scn.write_text(scenario_text(g))
    box = (10, 5, 80, 30)
    sim = ea.Simulation(X, Y).load_text(scenario_text(g))
    # frame f is drawn behind key f; frame 0 shows what --paint asked for: vorticity:3 -> pressure (1000) -> speed (10) -> unpainted -> vorticity:3, no key
    start = [(ea.PAINT_VORTICITY, 3.0), (ea.PAINT_PRESSURE, 1000.0), (ea.PAINT_SPEED, 10.0), None, (ea.PAINT_VORTICITY, 3.0), (ea.PAINT_VORTICITY, 3.0)]
    want_paint = []
    for f in range(6):
        if f:
            sim.step()
        if f == 0:
            plain0 = sim.render_view(box, 49, 19)
        want_paint.append(_composition(sim, box, True, 49, 19, *start[f]) if start[f] else sim.render_view(box, 49, 19))
    sim.close()
    base = [EXE, "--dump", "--window", "49x19", "--frames", "5", "--view", "%d,%d,%d,%d" % box]
    # the scale given with --paint replaces its field's default; the others keep 1000 and 10
    run = subprocess.run(base + ["--paint", "vorticity:3", "--keys", "vvvv.", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert dumped_frames(run.stdout) == want_paint
    # without --paint the cycle starts unpainted, at the defaults: vorticity at 1
    sim = ea.Simulation(X, Y).load_text(scenario_text(g))
    sim.step()
    first = _composition(sim, box, True, 49, 19, ea.PAINT_VORTICITY, 1.0)
    sim.close()
    run = subprocess.run(base + ["--keys", "v", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    got = dumped_frames(run.stdout)
    assert got[1] == first and got[0] == plain0
    # v is a view key only: with --fit it does nothing
    run = subprocess.run([EXE, "--dump", "--window", "49x19", "--frames", "2", "--fit", "--keys", "vv", str(scn)], capture_output=True, timeout=120)
    run2 = subprocess.run([EXE, "--dump", "--window", "49x19", "--frames", "2", "--fit", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0 and run.stdout == run2.stdout
