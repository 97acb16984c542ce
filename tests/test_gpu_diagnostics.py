"""euler_diagnostics on the GPU (docs/diagnostics.md): the record of the device reduction against the numpy restatement (tests/diagnostics_ref.py) of
the fields read back through euler_get_field - every field exactly equal, max_div and max_speed2 bit for bit - over the five scenarios, grids that
take the four-cells-per-lane and the one-cell-per-lane path, boxes that cut a lane's group at either edge, sit inside one tile or span idle tiles,
with and without the tile map; planted non-finite values and counts; that the pass leaves no trace in the state; `euler --stats`."""
import subprocess

import numpy as np
import pytest

import diagnostics_ref as ref
import euler_amd as ea
from euler_amd import scenarios
from golden_util import SCENARIOS, X, Y, load, scenario_text
from observer_util import EULER_EINVAL, EULER_ESTATE, EXE, no_trace_pair

pytestmark = pytest.mark.gpu


def terms_of(sim):
    return ref.cell_terms(*(sim.get(f) for f in (ea.F_SOLID, ea.F_COUNT, ea.F_U, ea.F_V)))


def check(sim, boxes, what, terms=None):
    terms = terms or terms_of(sim)
    for box in boxes:
        got, want = sim.diagnostics_record(box), ref.reduce_box(terms, box)
        assert got.dtype == ea.DIAG_DTYPE and got.shape == ()
        bad = ref.mismatches(got, want)
        if box is None or bad:
            print("%s box %s: fluid %d of %d cells, markers %d, max |d| %g, max speed^2 %g, non-finite %d; fields that differ: %s" %
                  (what, box, int(want["fluid"]), int(want["cells"]), int(want["markers"]), float(want["max_div"]), float(want["max_speed2"]), int(want["nonfinite"]), bad or "none"))
        assert not bad, (what, box, bad)
    return terms


# ----------------------------------------------------------------------------- the surface
def test_refusals_and_the_buffer():
    sim = ea.Simulation(X, Y)
    with pytest.raises(ea.EulerError) as e:      # nothing loaded
        sim.diagnostics()
    assert e.value.code == EULER_ESTATE
    before = sim.hbm_bytes()
    sim.load_text(scenario_text(load("basic_frames.npz")))
    for box in ((0, 1, 5, 5), (1, 0, 5, 5), (1, 1, X - 1, 5), (1, 1, 5, Y - 1), (6, 1, 5, 5), (1, 6, 5, 5), (-3, -3, -1, -1), (X, Y, X + 5, Y + 5)):
        with pytest.raises(ea.EulerError) as e:
            sim.diagnostics(box)
        assert e.value.code == EULER_EINVAL, box
    rec = np.zeros((), ea.DIAG_DTYPE)
    for nbytes in (0, 87, 89, 176):
        assert sim.L.euler_diagnostics(sim.h, 1, 1, 5, 5, rec.ctypes.data, nbytes) == EULER_EINVAL, nbytes
    assert sim.L.euler_diagnostics(sim.h, 1, 1, 5, 5, None, 88) == EULER_EINVAL
    assert sim.hbm_bytes() == before                      # a handle that never ran it allocates nothing
    assert sim.L.euler_diagnostics(sim.h, 1, 1, 5, 5, rec.ctypes.data, 88) == 0 and rec["cells"] == 25
    assert sim.hbm_bytes() == before + 88
    d = sim.diagnostics()
    assert sim.hbm_bytes() == before + 88
    want = ref.reduce_box(terms_of(sim))
    assert set(d) == set(ea.DIAG_DTYPE.names) | set(ea.DIAG_VALUES)
    assert all(d[n] == want[n] for n in ea.DIAG_DTYPE.names) and all(d[k] == v for k, v in ref.derive(want).items())
    assert d["fluid"] > 0 and d["markers"] == sim.stats().n_markers and d["crowded"] == 0      # the seeding: every marker lies in a fluid cell, four to a cell
    sim.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:
        slab.diagnostics()
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()


# ----------------------------------------------------------------------------- the five scenarios
@pytest.mark.parametrize("scn", SCENARIOS)
def test_scenarios_at_native_size(scn):
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenario_text(load(scn + "_frames.npz")))
    boxes = ref.boxes(X, Y, 1)
    for frame in range(31):
        if frame in (0, 1, 30):
            t = check(sim, boxes, "%s frame %d" % (scn, frame))
            assert t["fluid"].any()
        sim.step()
    sim.close()


def test_planted_values_and_counts():
    """NaN / inf / huge values in u, counts 8 and 255 (euler_set_field): a NaN is counted once and adds nothing, an infinity saturates"""
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenario_text(load("block_frames.npz")))
    for _ in range(5):
        sim.step()
    u, count = sim.get(ea.F_U), sim.get(ea.F_COUNT)
    wet = np.argwhere((count > 0) & (sim.get(ea.F_SOLID) == 0))
    assert len(wet) > 40
    for k, (y, x) in enumerate(wet[:: max(1, len(wet) // 40)]):
        u[y, x] = (np.nan, np.inf, -np.inf, 1e30, -3e38)[k % 5]
        count[y, x + 1 if x + 1 < X - 1 else x] = (8, 255, 7)[k % 3]
    sim.set(ea.F_U, u); sim.set(ea.F_COUNT, count)
    t = check(sim, ref.boxes(X, Y, 2), "planted values")
    whole = ref.reduce_box(t)
    assert whole["nonfinite"] > 0 and np.isinf(whole["max_div"]) and np.isinf(whole["max_speed2"]) and whole["count_max"] == 255 and whole["crowded"] > 0
    sim.close()


def test_ragged_small_grid_in_motion():
    """one cell per lane (X % 4 != 0) on water that has hit the floor - the large ragged grid below is still falling, its divergence all but zero - and
    with planted values; 70 x 9 and 9 x 200: boxes narrower than a wave and taller than several row segments"""
    sim = ea.Simulation(101, 43, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenario_text(load("block_frames.npz")), upscale=True)
    for _ in range(30):
        sim.step()
    t = check(sim, ref.boxes(101, 43, 5), "101x43 frame 30")
    assert ref.reduce_box(t)["max_div"] > 0.01 and ref.reduce_box(t)["ke_hi"] > 0
    u = sim.get(ea.F_U)
    wet = np.argwhere(t["fluid"])
    for k, (y, x) in enumerate(wet[:: max(1, len(wet) // 30)]):
        u[y, x] = (np.nan, np.inf, -np.inf, 1e30)[k % 4]
    sim.set(ea.F_U, u)
    t = check(sim, ref.boxes(101, 43, 6), "101x43 planted")
    assert ref.reduce_box(t)["nonfinite"] > 0
    sim.close()
    for size in ((70, 9), (9, 200)):
        sim = ea.Simulation(*size, dot_mode=ea.DOT_SEQUENTIAL).load_text("\n".join(["0" * 40] * 30), upscale=True)
        rng = np.random.default_rng(7)
        sim.set(ea.F_U, rng.standard_normal(size[::-1]).astype(np.float32)); sim.set(ea.F_V, rng.standard_normal(size[::-1]).astype(np.float32))
        t = check(sim, ref.boxes(*size, 7), "%dx%d random u, v" % size)
        assert ref.reduce_box(t)["fluid"] > 0 and ref.reduce_box(t)["div_l1"] > 0
        sim.close()


# ----------------------------------------------------------------------------- four cells per lane (X % 4 == 0) and one (a ragged X)
@pytest.mark.parametrize("size", [(1000, 700), (1031, 517)])
def test_aligned_and_ragged_grids(size):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50).load_text(scenarios.dam_break(), upscale=True)
    boxes = ref.boxes(*size, 3)
    check(sim, boxes, "%dx%d frame 0" % size)
    for _ in range(8):
        sim.step()
    t = check(sim, boxes, "%dx%d" % size)
    assert ref.reduce_box(t)["max_speed2"] > 0.25      # (some frames in: the column is falling)
    sim.set_option(ea.OPT_NO_TILE_MAP, 1)
    check(sim, boxes, "%dx%d, no tile map" % size, t)
    sim.close()


def test_1024_dam_break_with_and_without_the_tile_map():
    sim = ea.Simulation(1024, 1024, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=20).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(25):
        sim.step()
    t = terms_of(sim)
    wet_tiles = t["fluid"].reshape(16, 64, 16, 64).any(axis=(1, 3))
    assert 0 < wet_tiles.sum() < 256      # some tiles hold water, some are idle
    ty, tx = (int(k) for k in np.argwhere(~wet_tiles)[-1])      # a box without water, over more than one idle tile where there is room
    dry = (max(1, 64 * tx - 30), max(1, 64 * ty - 30), min(1022, 64 * tx + 62), min(1022, 64 * ty + 62))
    dry = dry if ref.reduce_box(t, dry)["fluid"] == 0 else (max(1, 64 * tx), max(1, 64 * ty), min(1022, 64 * tx + 63), min(1022, 64 * ty + 63))
    boxes = ref.boxes(1024, 1024, 4) + [dry]
    for key in (0, 1):
        sim.set_option(ea.OPT_NO_TILE_MAP, key)
        check(sim, boxes, "1024^2 dam break, no_tile_map=%d" % key, t)
        got = sim.diagnostics_record(dry)
        assert got["cells"] == (dry[2] - dry[0] + 1) * (dry[3] - dry[1] + 1) and all(got[n] == 0 for n in ea.DIAG_DTYPE.names[1:]), key
    whole = ref.reduce_box(t)
    assert whole["max_div"] > 0 and whole["div_l1"] > 0 and whole["ke_hi"] > 0      # 20 iterations do not resolve the pressure: the divergence the doc speaks of
    sim.close()


# ----------------------------------------------------------------------------- no lasting state
def _pair(options=(), **kw):
    def make():
        s = ea.Simulation(256, 256, **kw).load_text(scenarios.dam_break(), upscale=True)
        for k, v in options:
            s.set_option(k, v)
        return s

    def between_stages(s, st):      # (the count grid moves ahead of the tile map's next refresh here)
        check(s, [None, (70, 2, 77, 9), (5, 3, 250, 130)], "between the stages, after stage %d" % st)

    a, b = no_trace_pair(make, lambda s, stepped: s.diagnostics((5, 3, 250, 130)) if stepped else s.diagnostics(), between_stages, frames=20, compare_every=20)
    assert a.stats().total_substeps >= 20
    check(b, [None], "after the pair")
    a.close(); b.close()


def test_the_pass_leaves_no_trace():
    _pair(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=30)


def test_no_trace_with_maccormack():
    _pair(options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)), dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=30)


def test_no_trace_with_viscosity():
    _pair(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=30, viscosity=0.5)


def test_no_trace_with_the_multilevel_solver():
    _pair(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=400)


# ----------------------------------------------------------------------------- the front end
def test_cli_stats(tmp_path):
    g = load("basic_frames.npz")
    scn = tmp_path / "basic.txt"
    scn.write_text(scenario_text(g))
    sim = ea.Simulation(X, Y).load_text(scenario_text(g))
    lines, plain = {}, []
    for f in range(101):
        if f:
            sim.step()
        plain.append(sim.draw(98, 38))
        lines[f] = ref.csv_line(f, sim.stats(), sim.diagnostics_record())
    sim.close()
    out = tmp_path / "stats.csv"
    base = [EXE, "--dump", "--frames", "100"]
    run = subprocess.run(base + ["--stats", str(out), str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert out.read_text().split("\n") == [ref.HEADER] + [lines[f] for f in range(101)] + [""]
    frames = [c.split(b"\n", 1)[1][: int(c.split(b"(")[1].split()[0])] for c in run.stdout.split(b"--- frame ")[1:]]
    assert frames == plain      # the dumped frames are what they are without the flag
    run = subprocess.run(base + ["--stats", str(out), "--stats-every", "7", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert out.read_text().split("\n") == [ref.HEADER] + [lines[f] for f in range(0, 101, 7)] + [""]
    # together with --fit and --ppm
    run = subprocess.run([EXE, "--dump", "--frames", "3", "--fit", "--ppm", str(tmp_path / "img_"), "--stats", str(out), str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert out.read_text().split("\n") == [ref.HEADER] + [lines[f] for f in range(4)] + [""]
    assert len(list(tmp_path.glob("img_*.ppm"))) == 4
    # refusals: usage, status 1; a write error ends the run with status 1
    run = subprocess.run(base + ["--stats", str(out), "--stats-every", "0", str(scn)], capture_output=True, timeout=60)
    assert run.returncode == 1 and b"--stats FILE" in run.stderr
    run = subprocess.run(base + ["--stats", str(tmp_path / "no_such_dir" / "s.csv"), str(scn)], capture_output=True, timeout=60)
    assert run.returncode == 1 and b"cannot write" in run.stderr
