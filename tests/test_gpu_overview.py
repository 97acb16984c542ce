"""euler_overview on the GPU (docs/overview.md): the records of the device reduction against the numpy restatement (tests/overview_ref.py)
of the fields read back through euler_get_field - every field exactly equal, max_speed2 bit for bit - over the five scenarios, shapes that
divide nothing, large grids with and without the tile map; that the pass leaves no trace in the state; the fit-to-window frame and the
`euler` front end's --fit / --ppm."""
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import overview_ref as ref
from euler_amd import scenarios
from golden_util import SCENARIOS, X, Y, load, scenario_text
from observer_util import DYE, EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames, no_trace_pair, read_back
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu


def check(sim, dye, shapes, what, state=None):
    state = state or read_back(sim, dye)
    for (w, h) in shapes:
        got = sim.overview(w, h)
        assert got.shape == (h, w) and got.dtype == ea.OVERVIEW_DTYPE
        want = ref.overview_ref(*state, w, h)
        bad = ref.mismatches(got, want)
        print("%s %dx%d: water %d of %d cells, max speed^2 %g, fields that differ: %s" % (what, w, h, int(want["water"].sum()), int(want["cells"].sum()), float(want["max_speed2"].max()), bad or "none"))
        assert not bad, (what, w, h, bad)
    return state


# ----------------------------------------------------------------------------- the surface
def test_surface():
    sim = ea.Simulation(X, Y)
    with pytest.raises(ea.EulerError) as e:      # nothing loaded
        sim.overview(10, 10)
    assert e.value.code == EULER_ESTATE
    before = sim.hbm_bytes()
    sim.load_text(scenario_text(load("basic_frames.npz")))
    for (w, h) in ((0, 5), (5, 0), (-1, 5), (X - 1, 5), (5, Y - 1), (X - 1, Y - 1)):
        with pytest.raises(ea.EulerError) as e:
            sim.overview(w, h)
        assert e.value.code == EULER_EINVAL, (w, h)
    buf = np.zeros(50, ea.OVERVIEW_DTYPE)
    for nbytes in (0, 48 * 50 - 1, 48 * 50 + 48, 48):
        assert sim.L.euler_overview(sim.h, 10, 5, buf.ctypes.data, nbytes) == EULER_EINVAL, nbytes
    assert sim.L.euler_overview(sim.h, 10, 5, None, 48 * 50) == EULER_EINVAL
    assert sim.hbm_bytes() == before                      # a handle that never ran it allocates nothing
    assert sim.L.euler_overview(sim.h, 10, 5, buf.ctypes.data, 48 * 50) == 0
    assert sim.hbm_bytes() == before + 48 * 50
    state = read_back(sim, False)
    check(sim, False, [(3, 2), (98, 38), (7, 5), (98, 38), (1, 1), (49, 19)], "growing and shrinking", state)
    assert sim.hbm_bytes() == before + 48 * 98 * 38
    n = ea.C.c_int32(0)
    for (wx, wy) in ((0, 5), (5, 0), (-3, -3)):
        assert sim.L.euler_render_fit(sim.h, wx, wy, None, 0, ea.C.byref(n)) == EULER_EINVAL
    assert sim.render_fit(1000, 1000) == sim.draw(1000, 1000)      # the window clipped to the interior: one cell per glyph
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:
        slab.overview(10, 10)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    with pytest.raises(ea.EulerError) as e:
        slab.render_fit(10, 10)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()


# ----------------------------------------------------------------------------- the five scenarios
@pytest.mark.parametrize("rainbow", [False, True])
@pytest.mark.parametrize("scn", SCENARIOS)
def test_scenarios_at_native_size(scn, rainbow):
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL, rainbow=rainbow).load_text(scenario_text(load(scn + "_frames.npz")))
    for _ in range(60):
        sim.step()
    st = check(sim, rainbow, [(98, 38), (49, 19), (33, 13), (7, 5), (1, 1)], "%s rainbow=%d" % (scn, rainbow))
    assert (st[2] > 0).any()
    if not rainbow:
        assert (sim.overview(7, 5)["dye"] == 0).all()
    sim.close()


def test_nan_and_out_of_range_values_follow_the_record():
    """a NaN speed term is skipped, a NaN dye counts 0, dye beyond [0, 1] is clamped"""
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True).load_text(scenario_text(load("block_frames.npz")))
    for _ in range(5):
        sim.step()
    u, r = sim.get(ea.F_U), sim.get(ea.F_DYE_R)
    wet = np.argwhere(sim.get(ea.F_COUNT) > 0)
    for k, (y, x) in enumerate(wet[:: max(1, len(wet) // 40)]):
        u[y, x] = np.nan if k % 2 else np.inf
        r[y, x] = (np.nan, -0.5, 1.5, np.inf)[k % 4]
    sim.set(ea.F_U, u); sim.set(ea.F_DYE_R, r)
    check(sim, True, [(98, 38), (33, 13), (1, 1)], "non-finite values")
    sim.close()


# ----------------------------------------------------------------------------- shapes that divide nothing
@pytest.mark.parametrize("size", [(1000, 700), (1031, 517)])
def test_non_dividing_shapes(size):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50, rainbow=True).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(8):
        sim.step()
    st = check(sim, True, [(997, 511), (256, 256), (80, 24), (3, 2)], "%dx%d" % size)
    assert np.abs(st[4]).max() > 0.5      # (some frames in: the column is falling)
    sim.set_option(ea.OPT_NO_TILE_MAP, 1)
    check(sim, True, [(256, 256), (3, 2)], "%dx%d, no tile map" % size, st)
    sim.close()


# ----------------------------------------------------------------------------- large grids, the tile map
def _large(sim, dye, what):
    state = read_back(sim, dye)
    shapes = [(1024, 1024), (200, 50)]
    want = [ref.overview_ref(*state, w, h) for (w, h) in shapes]
    del state
    for key in (0, 1):
        sim.set_option(ea.OPT_NO_TILE_MAP, key)
        for (w, h), wnt in zip(shapes, want):
            bad = ref.mismatches(sim.overview(w, h), wnt)
            print("%s %dx%d no_tile_map=%d: water %d, fields that differ: %s" % (what, w, h, key, int(wnt["water"].sum()), bad or "none"))
            assert not bad, (what, w, h, key, bad)
    return want


def test_4096_dam_break_in_motion():
    sim = ea.Simulation(4096, 4096, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=20, rainbow=True).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(30):
        sim.step()
    want = _large(sim, True, "4096^2 dam break")
    assert want[0]["max_speed2"].max() > 1.0 and 0 < want[1]["water"].sum() < 4094 * 4094 // 2
    sim.close()


def test_8192_half_tank():
    sim = ea.Simulation(8192, 8192, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=20).load_half_tank()
    for _ in range(3):
        sim.step()
    want = _large(sim, False, "8192^2 half tank")
    assert want[1]["water"].sum() > 8190 * 8190 // 3
    sim.close()


# ----------------------------------------------------------------------------- no lasting state
def _pair(scn, frames=40, options=(), **kw):
    text = scenario_text(load(scn + "_frames.npz"))

    def make():
        s = ea.Simulation(X, Y, **kw).load_text(text)
        for k, v in options:
            s.set_option(k, v)
        return s

    def between_stages(s, st):
        s.overview(49, 19)
        s.render_fit(20, 10)

    fields = STATE_FIELDS + (DYE if kw.get("rainbow") else ())
    for s in no_trace_pair(make, lambda s, stepped: s.overview(98, 38) if stepped else s.overview(33, 13), between_stages, fields, frames, compare_every=1):
        s.close()


@pytest.mark.parametrize("scn", SCENARIOS)
def test_the_pass_leaves_no_trace(scn):
    _pair(scn, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True)


def test_no_trace_with_maccormack():
    _pair("filter", options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)), dot_mode=ea.DOT_SEQUENTIAL, rainbow=True)


def test_no_trace_with_viscosity():
    _pair("waterfall", dot_mode=ea.DOT_SEQUENTIAL, viscosity=0.5)


def test_no_trace_with_the_multilevel_solver():
    _pair("basic", dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=400)


def test_no_trace_on_a_large_lean_grid():
    """1024^2: the grid passes run in their lean forms (tile map, zero_bounds four cells per thread), whose validity flags the pass must not touch"""
    kw = dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=30)
    a = ea.Simulation(2048, 2048, **kw).load_text(scenarios.dam_break(), upscale=True)
    b = ea.Simulation(2048, 2048, **kw).load_text(scenarios.dam_break(), upscale=True)
    for f in range(12):
        b.overview(200, 50)
        a.step(); b.step()
        b.overview(1024, 1024)
    for fld in (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP, ea.F_COUNT, ea.F_MARKERS):
        assert_bits(b.get(fld), a.get(fld), "field %d" % fld)
    a.close(); b.close()


# ----------------------------------------------------------------------------- the fit-to-window frame
def test_render_fit_at_one_cell_per_glyph_is_draw():
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenario_text(load("waterfall_frames.npz")))
    for f in range(100):
        assert sim.render_fit(X - 2, Y - 2) == sim.draw(X - 2, Y - 2), f
        sim.step()
    sim.close()


def test_render_fit_is_the_text_of_the_records():
    for rainbow in (False, True):
        sim = ea.Simulation(300, 200, dot_mode=ea.DOT_TREE, rainbow=rainbow).load_text(scenarios.dam_break(), upscale=True)
        for _ in range(10):
            sim.step()
        for (wx, wy) in ((98, 38), (49, 19), (500, 30)):
            w, h = min(wx, 298), min(wy, 198)
            assert sim.render_fit(wx, wy) == ea.overview_text(sim.overview(w, h), rainbow=rainbow), (rainbow, wx, wy)
        sim.close()


# ----------------------------------------------------------------------------- the front end
def test_cli_fit_and_ppm(tmp_path):
    g = load("basic_frames.npz")
    scn = tmp_path / "basic.txt"
    scn.write_text(scenario_text(g))
    sim = ea.Simulation(X, Y).load_text(scenario_text(g))
    fit, plain, images = [], [], {}
    for f in range(6):
        if f:
            sim.step()
        fit.append(sim.render_fit(49, 19))
        plain.append(sim.draw(49, 19))
        if f % 2 == 0:
            images[f] = sim.overview(40, 16)
    sim.close()
    base = [EXE, "--dump", "--window", "49x19", "--frames", "5"]
    run = subprocess.run(base + ["--fit", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert dumped_frames(run.stdout) == fit
    # without the new flags: the frames of draw, as before
    run = subprocess.run(base + [str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0 and dumped_frames(run.stdout) == plain and plain != fit
    # --ppm: frames / every + 1 files, the bytes of write_ppm(overview_rgb(...)) of the same state; the dumped frames unchanged
    prefix = str(tmp_path / "img_")
    run = subprocess.run(base + ["--ppm", prefix, "--ppm-size", "40x16", "--ppm-every", "2", "--ppm-mode", "speed:2.5", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert dumped_frames(run.stdout) == plain
    assert sorted(p.name for p in tmp_path.glob("img_*.ppm")) == ["img_%06d.ppm" % f for f in (0, 2, 4)]
    for f, px in images.items():
        want = tmp_path / "want.ppm"
        ea.write_ppm(str(want), ea.overview_rgb(px, ea.IMAGE_SPEED, 2.5))
        assert (tmp_path / ("img_%06d.ppm" % f)).read_bytes() == want.read_bytes(), f
    # defaults: the whole interior (both sides <= 1024: one cell per pixel here), coverage without --rainbow and the dye with it
    for flags, mode in (([], ea.IMAGE_COVERAGE), (["--rainbow"], ea.IMAGE_DYE)):
        prefix = str(tmp_path / ("d%d_" % mode))
        run = subprocess.run([EXE, "--dump", "--frames", "1", "--fit", "--ppm", prefix] + flags + [str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0, run.stderr.decode()
        s2 = ea.Simulation(X, Y, rainbow=bool(flags)).load_text(scenario_text(g))
        s2.step()
        want = tmp_path / "want.ppm"
        ea.write_ppm(str(want), ea.overview_rgb(s2.overview(X - 2, Y - 2), mode))
        assert (tmp_path / ("d%d_000001.ppm" % mode)).read_bytes() == want.read_bytes()
        s2.close()
    # refusals: usage, status 1
    for bad in (["--ppm-mode", "heat"], ["--ppm-mode", "speed:0"], ["--ppm-mode", "speed:x"], ["--ppm-every", "0"], ["--ppm-size", "99x10"], ["--ppm-size", "10x39"], ["--ppm-size", "0x5"]):
        run = subprocess.run(base + ["--ppm", prefix] + bad + [str(scn)], capture_output=True, timeout=60)
        assert run.returncode == 1 and b"--ppm PREFIX" in run.stderr and b"--fit" in run.stderr, bad
    # a write error ends the run with status 1
    run = subprocess.run(base + ["--ppm", str(tmp_path / "no_such_dir" / "f"), str(scn)], capture_output=True, timeout=60)
    assert run.returncode == 1 and b"cannot write" in run.stderr
