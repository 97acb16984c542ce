"""The pan-and-zoom viewport on the GPU (docs/viewport.md): euler_overview_box's records and euler_marker_raster's counts against the numpy
restatement (tests/viewport_ref.py) of the fields and markers read back - every field exactly equal, max_speed2 bit for bit - over the five
scenarios, aligned and ragged large grids with and without the tile map, thin grids; the refusals; that the calls leave no trace in the state;
euler_render_view and the `euler` front end's --view."""
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import overview_ref as ref
import viewport_ref as vref
from euler_amd import scenarios
from golden_util import SCENARIOS, X, Y, load, scenario_text
from observer_util import DYE, EULER_EINVAL, EULER_ESTATE, EXE, STATE_FIELDS, dumped_frames, no_trace_pair, read_back

pytestmark = pytest.mark.gpu


def cases(Xg, Yg, seed, extra=()):
    """[(box, W, H)]: the whole interior, a one-cell, a one-row and a one-column box, 20 seeded random boxes with random W <= Bw, H <= Bh (the first
    with x0 % 4 != 0 and x1 % 4 != 3), and whatever the grid adds"""
    rng = np.random.default_rng(seed)
    xi, yi = Xg - 2, Yg - 2
    out = [((1, 1, xi, yi), min(xi, 33), min(yi, 13)), ((1, 1, xi, yi), xi, yi),
           ((xi // 2 + 1, yi // 2 + 1, xi // 2 + 1, yi // 2 + 1), 1, 1), ((1, yi, xi, yi), max(1, xi // 3), 1), ((xi, 1, xi, yi), 1, max(1, yi // 2))]
    while len(out) < 25:
        xs, ys = np.sort(rng.integers(1, xi + 1, 2)), np.sort(rng.integers(1, yi + 1, 2))
        box = (int(xs[0]), int(ys[0]), int(xs[1]), int(ys[1]))
        if len(out) == 5 and (box[0] % 4 == 0 or box[2] % 4 == 3):
            continue
        bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
        full = rng.random() < 0.25      # (one cell per record now and then)
        out.append((box, bw if full else int(rng.integers(1, bw + 1)), bh if full else int(rng.integers(1, bh + 1))))
    return out + list(extra)


def check_boxes(sim, dye, todo, what, state=None):
    state = state or read_back(sim, dye)
    for box, w, h in todo:
        got = sim.overview(w, h, box=box)
        assert got.shape == (h, w) and got.dtype == ea.OVERVIEW_DTYPE
        want = vref.overview_box_ref(*state, box, w, h)
        bad = ref.mismatches(got, want)
        if bad:
            print("%s box %s %dx%d: water %d of %d cells, fields that differ: %s" % (what, box, w, h, int(want["water"].sum()), int(want["cells"].sum()), bad))
        assert not bad, (what, box, w, h, bad)
        if box == (1, 1, sim.X - 2, sim.Y - 2):      # the whole interior: euler_overview record for record
            assert not ref.mismatches(got, sim.overview(w, h)), (what, w, h)
    return state


def check_rasters(sim, todo, what, markers=None):
    m = sim.get(ea.F_MARKERS) if markers is None else markers
    for box, scale in todo:
        got = sim.marker_raster(box, scale)
        want = vref.raster_ref(m, box, scale)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got, want), (what, box, scale, int(got.sum()), int(want.sum()))
    return m


def check_counts(sim, what):
    """At a frame boundary the scale-1 raster of the whole interior, mod 256 (the count grid is uint8 and wraps), is EULER_F_COUNT on the cells that are
    neither solid nor sink (markers there are deleted by the refresh, and the count of such a cell is whatever the refresh left).  Where it cannot
    hold: the source stage counts a new marker in its source cell at (x + rx, y + ry) with rx, ry drawn from the CLOSED [0, 1], and the seeding
    jitter is drawn from the closed [0, 0.5]: a draw of exactly 1.0 (2^-32 per draw; none in these runs) puts the marker on the next cell's edge."""
    box = (1, 1, sim.X - 2, sim.Y - 2)
    ras = sim.marker_raster(box, 1)
    solid, sink, count = (sim.get(f)[sim.Y - 2:0:-1, 1:sim.X - 1] for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT))
    open_ = (solid == 0) & (sink == 0)
    assert np.array_equal((ras % 256)[open_], count[open_].astype(np.uint32)), what
    return ras


# ----------------------------------------------------------------------------- the surface
def test_refusals():
    sim = ea.Simulation(X, Y)
    n = ea.C.c_int32(0)
    for call in (lambda: sim.overview(5, 5, box=(1, 1, 10, 10)), lambda: sim.marker_raster((1, 1, 10, 10), 1), lambda: sim.render_view((1, 1, 10, 10), 20, 20)):
        with pytest.raises(ea.EulerError) as e:      # nothing loaded
            call()
        assert e.value.code == EULER_ESTATE
    sim.load_text(scenario_text(load("basic_frames.npz")))
    before = sim.hbm_bytes()
    bad_boxes = ((0, 1, 10, 10), (1, 0, 10, 10), (1, 1, X - 1, 10), (1, 1, 10, Y - 1), (11, 1, 10, 10), (1, 11, 10, 10), (-5, -5, -1, -1))
    for box in bad_boxes:
        for call in (lambda: sim.overview(1, 1, box=box), lambda: sim.marker_raster(box, 1), lambda: sim.render_view(box, 20, 20)):
            with pytest.raises(ea.EulerError) as e:
                call()
            assert e.value.code == EULER_EINVAL, box
    for (w, h) in ((11, 5), (5, 6), (0, 5), (5, 0), (-1, 5)):      # box of 10 x 5 cells
        with pytest.raises(ea.EulerError) as e:
            sim.overview(w, h, box=(3, 3, 12, 7))
        assert e.value.code == EULER_EINVAL, (w, h)
    buf = np.zeros(50, ea.OVERVIEW_DTYPE)
    for nbytes in (0, 48 * 50 - 1, 48 * 50 + 48, 48):
        assert sim.L.euler_overview_box(sim.h, 3, 3, 12, 7, 10, 5, buf.ctypes.data, nbytes) == EULER_EINVAL, nbytes
    assert sim.L.euler_overview_box(sim.h, 3, 3, 12, 7, 10, 5, None, 48 * 50) == EULER_EINVAL
    for scale in (0, 3, 5, 32, -2):
        with pytest.raises(ea.EulerError) as e:
            sim.marker_raster((3, 3, 12, 7), scale)
        assert e.value.code == EULER_EINVAL, scale
    ras = np.zeros(10 * 5 * 4, np.uint32)
    for nbytes in (0, ras.nbytes - 4, ras.nbytes + 4, 4):
        assert sim.L.euler_marker_raster(sim.h, 3, 3, 12, 7, 2, ras.ctypes.data, nbytes) == EULER_EINVAL, nbytes
    assert sim.L.euler_marker_raster(sim.h, 3, 3, 12, 7, 2, None, ras.nbytes) == EULER_EINVAL
    for (wx, wy) in ((0, 5), (5, 0), (-3, -3)):
        assert sim.L.euler_render_view(sim.h, 3, 3, 12, 7, wx, wy, None, 0, ea.C.byref(n)) == EULER_EINVAL
    assert sim.hbm_bytes() == before                      # a refused call allocates nothing
    assert sim.marker_raster((3, 3, 12, 7), 2).shape == (10, 20)
    assert sim.hbm_bytes() == before + 4 * 200
    sim.marker_raster((3, 3, 12, 7), 1)
    assert sim.hbm_bytes() == before + 4 * 200          # (shrinking keeps the buffer)
    sim.overview(10, 5, box=(3, 3, 12, 7))
    sim.overview(2, 2)                                    # one buffer for both overview calls
    assert sim.hbm_bytes() == before + 4 * 200 + 48 * 50
    sim.close()
    big = ea.Simulation(300, 300).load_text(scenarios.dam_break(), upscale=True)      # W * H > 2^24
    for box, scale in (((1, 1, 256, 257), 16), ((1, 1, 257, 256), 16), ((1, 1, 298, 298), 16), ((2, 2, 290, 228), 16)):
        with pytest.raises(ea.EulerError) as e:
            big.marker_raster(box, scale)
        assert e.value.code == EULER_EINVAL, (box, scale)
    got = big.marker_raster((1, 1, 256, 256), 16)      # exactly 2^24
    assert got.shape == (4096, 4096) and np.array_equal(got, vref.raster_ref(big.get(ea.F_MARKERS), (1, 1, 256, 256), 16))
    big.close()
    slab = ea.Simulation(X, Y, slab=(0, 1))
    for call in (lambda: slab.overview(5, 5, box=(1, 1, 10, 10)), lambda: slab.marker_raster((1, 1, 10, 10), 1), lambda: slab.render_view((1, 1, 10, 10), 20, 20)):
        with pytest.raises(ea.EulerError) as e:
            call()
        assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    slab.close()


# ----------------------------------------------------------------------------- the five scenarios, frames 0 and 30
@pytest.mark.parametrize("scn", SCENARIOS)
def test_scenarios_at_native_size(scn):
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True).load_text(scenario_text(load(scn + "_frames.npz")))
    whole = (1, 1, X - 2, Y - 2)
    for frame in (0, 30):
        while sim.stats().frames < frame:
            sim.step()
        what = "%s frame %d" % (scn, frame)
        st = check_boxes(sim, True, cases(X, Y, 11 + frame), what)
        m = check_rasters(sim, [(whole, s) for s in vref.SCALES] + [(c[0], s) for c, s in zip(cases(X, Y, 5)[2:14], (1, 2, 4, 8, 16, 1, 2, 4, 8, 16, 4, 16))], what)
        one = check_counts(sim, what)
        assert one.sum() > 0 and (st[2] > 0).any()
        for s in vref.SCALES:      # every scale refines scale 1
            assert np.array_equal(sim.marker_raster(whole, s).reshape(Y - 2, s, X - 2, s).sum(axis=(1, 3)), one)
        assert len(m) == sim.stats().n_markers
    sim.close()


# ----------------------------------------------------------------------------- four cells per lane (X % 4 == 0) and one (a ragged X); the tile map
@pytest.mark.parametrize("size", [(1000, 700), (1031, 517)])
def test_aligned_and_ragged_grids(size):
    sim = ea.Simulation(*size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50, rainbow=True).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(8):
        sim.step()
    xi, yi = size[0] - 2, size[1] - 2
    dry = (xi - 290, 70, xi - 20, yi - 60)      # the right half of the tank: tiles without water
    extra = [((70, 70, 100, 100), 9, 7), ((70, 70, 100, 100), 31, 31),      # inside one 64 x 64 tile
             (dry, 40, 20), (dry, 1, 1),
             ((5, 3, xi - 90, yi - 9), 2, 1), ((1, 1, xi, yi), 1, 1), ((2, 2, xi - 1, yi - 1), 3, 2),      # tall boxes of few records: their rows are split between workgroups
             ((5, 130, 602, 400), 598, 271), ((6, 130, 601, 400), 300, 100), ((7, 1, 9, yi), 3, 5)]      # x0 % 4 = 1, 2, 3 with x1 % 4 = 2, 1, 1
    todo = cases(*size, 21, extra)
    st = check_boxes(sim, True, todo, "%dx%d" % size)
    assert np.abs(st[4]).max() > 0.5 and vref.overview_box_ref(*st, dry, 1, 1)["water"].sum() == 0
    sim.set_option(ea.OPT_NO_TILE_MAP, 1)
    check_boxes(sim, True, todo, "%dx%d, no tile map" % size, st)
    sim.set_option(ea.OPT_NO_TILE_MAP, 0)
    whole = (1, 1, xi, yi)
    check_rasters(sim, [(whole, 1), (whole, 2), ((70, 70, 100, 100), 16), ((5, 130, 602, 400), 4), (dry, 8), ((xi // 2, 1, xi // 2, yi), 16)], "%dx%d" % size)
    assert not sim.marker_raster(dry, 8).any()      # a box without markers: all zero
    check_counts(sim, "%dx%d" % size)
    sim.close()


def test_thin_grids_with_random_velocities():
    for size in ((70, 9), (9, 200)):
        sim = ea.Simulation(*size, dot_mode=ea.DOT_SEQUENTIAL).load_text("\n".join(["0" * 40] * 30), upscale=True)
        rng = np.random.default_rng(7)
        sim.set(ea.F_U, rng.standard_normal(size[::-1]).astype(np.float32)); sim.set(ea.F_V, rng.standard_normal(size[::-1]).astype(np.float32))
        st = check_boxes(sim, False, cases(*size, 31), "%dx%d random u, v" % size)
        assert (st[2] > 0).any()
        whole = (1, 1, size[0] - 2, size[1] - 2)
        check_rasters(sim, [(whole, s) for s in vref.SCALES], "%dx%d" % size)
        check_counts(sim, "%dx%d" % size)
        sim.close()


def test_rainbow_dam_break_256():
    sim = ea.Simulation(256, 256, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=50, rainbow=True).load_text(scenarios.dam_break(), upscale=True)
    for _ in range(10):
        sim.step()
    st = check_boxes(sim, True, cases(256, 256, 41), "256^2 rainbow")
    assert max(int(vref.overview_box_ref(*st, (1, 1, 254, 254), 1, 1)["dye"][0, 0, c]) for c in range(3)) > 0
    # the frame of a box: boxes of cells below one cell per glyph, the raster above - coloured on this handle
    for box, wx, wy in (((1, 1, 254, 254), 98, 38), ((20, 100, 68, 118), 98, 38), ((20, 100, 43, 108), 98, 38), ((30, 110, 33, 111), 98, 38), ((30, 110, 120, 111), 98, 38),
                        ((20, 100, 68, 118), 97, 38), ((20, 100, 68, 118), 1000, 1000)):
        bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
        s = vref.view_zoom(bw, bh, wx, wy)
        got = sim.render_view(box, wx, wy)
        if s:
            want = ea.view_text(sim.overview(bw, bh, box=box), sim.marker_raster(box, s), s, rainbow=True)
        else:
            want = ea.overview_text(sim.overview(min(wx, bw), min(wy, bh), box=box), rainbow=True)
        assert got == want and b"\x1b[38;2;" in got, (box, wx, wy, s)
    assert vref.view_zoom(49, 19, 98, 38) == 2 and vref.view_zoom(24, 9, 98, 38) == 4 and vref.view_zoom(4, 2, 98, 38) == 16 and vref.view_zoom(91, 2, 98, 38) == 0
    sim.close()


# ----------------------------------------------------------------------------- the raster
def test_raster_planted_and_shuffled_markers():
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenario_text(load("block_frames.npz")))
    for _ in range(10):
        sim.step()
    m0 = sim.get(ea.F_MARKERS)
    rng = np.random.default_rng(5)
    f = np.float32
    below = lambda a: np.nextafter(f(a), f(-np.inf))
    box = (13, 7, 52, 30)
    edge = np.array([(f(13), f(8.5)), (below(13), f(8.5)), (f(53), f(8.5)), (below(53), f(8.5)), (f(20.5), f(7)), (f(20.5), below(7)), (f(20.5), f(31)), (f(20.5), below(31)),
                     (np.nan, f(9)), (f(20), np.nan), (np.inf, f(9)), (f(20), -np.inf)], np.float32)
    point = np.tile(np.array([[20.3125, 9.71875]], np.float32), (1000, 1))      # 1000 markers on one point
    m = np.concatenate([m0[:1501], point[:400], edge, m0[1501:], point[400:]])
    if len(m) % 2 == 0:
        m = m[1:]      # an odd count (no multiple of 64): the last marker is loaded alone
    assert len(m) % 64 != 0
    sim.set_markers(m)
    todo = [(box, s) for s in vref.SCALES] + [((1, 1, X - 2, Y - 2), 1), ((20, 9, 20, 9), 16), ((20, 9, 20, 9), 1)]
    check_rasters(sim, todo, "planted", m)
    got = sim.marker_raster((20, 9, 20, 9), 16)
    assert got[15 - 11, 5] >= 1000      # floor(0.3125 * 16) = 5, floor(0.71875 * 16) = 11
    want = [sim.marker_raster(b, s) for b, s in todo]
    sim.set_markers(m[rng.permutation(len(m))])      # the same markers in another order: the same rasters
    for (b, s), w in zip(todo, want):
        assert np.array_equal(sim.marker_raster(b, s), w), (b, s)
    sim.close()


def test_render_view_of_the_whole_interior_is_draw():
    sim = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(scenario_text(load("waterfall_frames.npz")))
    for f in range(40):
        assert sim.render_view((1, 1, X - 2, Y - 2), 98, 38) == sim.draw(98, 38), f
        sim.step()
    sim.close()


# ----------------------------------------------------------------------------- no lasting state
def _pair(options=(), frames=20):
    def make():
        s = ea.Simulation(256, 256, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=30, rainbow=True).load_text(scenarios.dam_break(), upscale=True)
        for k, v in options:
            s.set_option(k, v)
        return s

    def look(s, stepped):
        if stepped:
            return
        s.overview(40, 20, box=(5, 3, 250, 130))
        s.marker_raster((20, 100, 68, 118), 4)
        s.render_view((20, 100, 43, 108), 98, 38)
        s.render_view((1, 1, 254, 254), 98, 38)

    def between_stages(s, st):
        look(s, False)
        check_rasters(s, [((1, 1, 254, 254), 1), ((20, 100, 68, 118), 8)], "after stage %d" % st)
        check_boxes(s, True, [((5, 3, 250, 130), 40, 20)], "after stage %d" % st)

    for s in no_trace_pair(make, look, between_stages, STATE_FIELDS + DYE, frames, compare_every=5):
        s.close()


def test_the_calls_leave_no_trace():
    _pair()


def test_no_trace_with_maccormack_and_rk2():
    _pair(options=((ea.OPT_ADVECT_MACCORMACK, 1), (ea.OPT_ADVECT_RK2, 1)))


# ----------------------------------------------------------------------------- the front end
def test_cli_view(tmp_path):
    g = load("block_frames.npz")
    scn = tmp_path / "block.txt"
    scn.write_text(scenario_text(g))
    start = (10, 5, 58, 23)
    base = [EXE, "--dump", "--window", "98x38", "--frames", "8"]
    view_flags = ["--view", "%d,%d,%d,%d" % start]
    for keys in ("l+-0hjk", "++kkhjl-"):      # (the second: the pans on a box that can move)
        sim = ea.Simulation(X, Y).load_text(scenario_text(g))
        box, boxes, view, plain, images = start, [], [], [], {}
        for f in range(9):
            if f:
                if f - 1 < len(keys):
                    box = vref.view_key(box, keys[f - 1], X - 2, Y - 2)
                sim.step()
            bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
            boxes.append(box)
            view.append(sim.render_view(box, 98, 38))
            plain.append(sim.draw(98, 38))
            images[f] = (None, sim.overview(min(20, bw), min(8, bh), box=box), sim.overview(bw, bh, box=box))
        sim.close()
        assert len(set(boxes)) >= 5 and len(set(view)) >= 5
        run = subprocess.run(base + view_flags + ["--keys", keys, str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0, run.stderr.decode()
        got = dumped_frames(run.stdout)
        assert len(got) == 9
        for f in range(9):
            assert got[f] == view[f], (keys, f, boxes[f])
        # without --view the keys do nothing: the frames of a run without them
        run = subprocess.run(base + ["--keys", keys, str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0 and dumped_frames(run.stdout) == plain
    run = subprocess.run(base + [str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0 and dumped_frames(run.stdout) == plain
    # --ppm with --view (the last key string): the box as it stands, --ppm-size clamped to it; by default the box at one cell per pixel (both sides <= 1024)
    for flags, pick in ((["--ppm-size", "20x8"], 1), ([], 2)):
        prefix = str(tmp_path / ("v%d_" % pick))
        run = subprocess.run(base + view_flags + ["--keys", keys, "--ppm", prefix] + flags + [str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0, run.stderr.decode()
        assert dumped_frames(run.stdout) == view
        for f in range(9):
            want = tmp_path / "want.ppm"
            ea.write_ppm(str(want), ea.overview_rgb(images[f][pick], ea.IMAGE_COVERAGE))
            assert (tmp_path / ("v%d_%06d.ppm" % (pick, f))).read_bytes() == want.read_bytes(), (pick, f)
    # refusals: usage, status 1
    for bad in (["--fit", "--view", "1,1,10,10"], ["--view", "0,1,10,10"], ["--view", "1,1,99,10"], ["--view", "5,1,4,10"], ["--view", "1,1,10"], ["--view", "1,1,10,10x"]):
        run = subprocess.run(base + bad + [str(scn)], capture_output=True, timeout=60)
        assert run.returncode == 1 and b"--view X0,Y0,X1,Y1" in run.stderr, bad
