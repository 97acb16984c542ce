"""The `euler` front end's passive tracers (docs/tracers.md): --tracer / --tracer-box / --emit / --tracers against a Python-driven handle doing the same, the CSV
byte for byte; --tracers-show with --fit, --view (both regimes, the key t) and --ppm against the Python composition of the same calls; the usage errors; and a
run without the new flags against the frames the handle draws."""
import subprocess

import numpy as np
import pytest

import euler_amd as ea
from golden_util import X, Y, load, scenario_text
from observer_util import EXE, dumped_frames

pytestmark = pytest.mark.gpu

FG, BG = (1.0, 0.9, 0.0), (0.25, 0.5, 1.0)


@pytest.fixture
def scn(tmp_path):
    path = tmp_path / "block.txt"
    path.write_text(scenario_text(load("block_frames.npz")))
    return path


def csv_lines(sim, frame):
    t = sim.time
    return "".join("%d,%.9g,%d,%.9g,%.9g,%.9g,%.9g,%.9g,%d,%d\n" % (frame, t, k, r["x"], r["y"], r["path"], r["age"], r["wet_time"], r["substeps"], r["flags"])
                   for k, r in enumerate(sim.tracers()))


def emit(sim, emitters, f):
    due = [p for p, every in emitters if f % every == 0]
    if due:
        sim.add_tracers(due)


def test_tracers_csv_against_a_python_driven_handle(scn, tmp_path):
    """seeds in command-line order in one add behind the load; every emitter due at frame F right before the step that produces it (F = 0: before frame 0 is drawn)"""
    emitters = [((25.5, 18.5), 1), ((40.5, 12.5), 3)]
    sim = ea.Simulation(X, Y).load_text(scn.read_text())
    sim.add_tracers(np.concatenate([[[10.5, 15.25]], ea.tracer_lattice((20, 12, 22, 13), 2), [[30.75, 20.5]], ea.tracer_lattice((50, 30, 50, 30), 1)]))
    frames, csv = [], "frame,time,index,x,y,path,age,wet_time,substeps,flags\n"
    for f in range(11):
        emit(sim, emitters, f)
        if f:
            sim.step()
        frames.append(sim.draw(98, 38))
        if f % 2 == 0:
            csv += csv_lines(sim, f)
    n = sim.n_tracers
    assert n == 1 + 24 + 1 + 1 + 11 + 4 and (sim.tracers()["path"] > 0).sum() > 20
    sim.close()
    out = tmp_path / "tracers.csv"
    flags = ["--tracer", "10.5,15.25", "--tracer-box", "20,12,22,13:2", "--tracer", "30.75,20.5", "--tracer-box", "50,30,50,30:1", "--emit", "25.5,18.5", "--emit", "40.5,12.5:3",
             "--tracers", str(out), "--tracers-every", "2"]
    run = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "10"] + flags + [str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert dumped_frames(run.stdout) == frames
    assert out.read_bytes() == csv.encode()
    # without any of the new flags every byte the command writes is what it was: the frames of a handle that never heard of tracers (they leave no trace: the same frames)
    plain = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "10", str(scn)], capture_output=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout == run.stdout and plain.stderr == run.stderr


def painted(sim, w, h, box, rainbow, paint=None):
    px = sim.overview(w, h, box)
    if paint:
        px = ea.flow_paint(sim.flow(w, h, box, pressure=paint[0] == ea.PAINT_PRESSURE), px, *paint)
    return ea.tracer_paint(sim.tracer_raster(box, w, h), px, FG, None if (rainbow or paint) else BG)


def shown_view(sim, box, wx, wy, rainbow=False):
    """euler_render_view's two regimes from the painted records"""
    bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
    if bw * 2 <= wx and bh * 2 <= wy:
        scale = 16
        while bw * scale > wx or bh * scale > wy:
            scale //= 2
        return ea.view_text(painted(sim, bw, bh, box, rainbow), sim.marker_raster(box, scale), scale, rainbow=True)
    return ea.overview_text(painted(sim, min(wx, bw), min(wy, bh), box, rainbow), rainbow=True)


SEEDS = ["--tracer-box", "10,12,40,25:1", "--emit", "45.5,20.5"]


def seeded(scn, rainbow=False):
    sim = ea.Simulation(X, Y, rainbow=rainbow).load_text(scn.read_text())
    sim.add_tracers(ea.tracer_lattice((10, 12, 40, 25), 1))
    return sim


@pytest.mark.parametrize("rainbow", [False, True])
def test_show_with_fit_and_ppm(scn, tmp_path, rainbow):
    sim = seeded(scn, rainbow)
    whole = (1, 1, X - 2, Y - 2)
    fit, images, fit_painted = [], [], []
    for f in range(7):
        emit(sim, [((45.5, 20.5), 1)], f)
        if f:
            sim.step()
        fit.append(ea.overview_text(painted(sim, 40, 15, whole, rainbow), rainbow=True))
        fit_painted.append(ea.overview_text(painted(sim, 40, 15, whole, rainbow, (ea.PAINT_SPEED, 10.0)), rainbow=True))
        if f % 3 == 0:
            images.append(ea.overview_rgb(painted(sim, 98, 38, whole, rainbow), ea.IMAGE_DYE))
    sim.close()
    assert len(set(fit)) >= 4 and fit != fit_painted      # (the scene moves; the paint shows)
    base = [EXE, "--dump", "--frames", "6", "--window", "40x15", "--fit", "--tracers-show"] + (["--rainbow"] if rainbow else []) + SEEDS
    prefix = str(tmp_path / "img")
    run = subprocess.run(base + ["--ppm", prefix, "--ppm-every", "3", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert dumped_frames(run.stdout) == fit
    for k, f in enumerate((0, 3, 6)):
        assert open("%s%06d.ppm" % (prefix, f), "rb").read() == b"P6\n98 38\n255\n" + images[k].tobytes(), f
    run = subprocess.run(base + ["--paint", "speed:10", str(scn)], capture_output=True, timeout=120)      # behind --paint: no blue for the rest
    assert run.returncode == 0 and dumped_frames(run.stdout) == fit_painted
    # --ppm alone is a picture mode too; the frames are then the plain ones
    run = subprocess.run([EXE, "--dump", "--frames", "0", "--window", "98x38", "--tracers-show", "--ppm", prefix + "b"] + (["--rainbow"] if rainbow else []) + SEEDS + [str(scn)],
                         capture_output=True, timeout=120)
    assert run.returncode == 0 and open(prefix + "b000000.ppm", "rb").read() == b"P6\n98 38\n255\n" + images[0].tobytes()


@pytest.mark.parametrize("box", [(3, 2, 96, 37), (20, 10, 43, 20)])      # larger than the window: boxes of cells; held twice: the magnified regime, one cell per record
def test_show_with_view_and_the_key_t(scn, box):
    keys = "..t.t"
    sim = seeded(scn)
    want, show = [], True
    for f in range(8):
        emit(sim, [((45.5, 20.5), 1)], f)
        if f:
            if f - 1 < len(keys) and keys[f - 1] == "t":
                show = not show
            sim.step()
        want.append(shown_view(sim, box, 60, 30) if show else sim.render_view(box, 60, 30))
    sim.close()
    run = subprocess.run([EXE, "--dump", "--frames", "7", "--window", "60x30", "--view", "%d,%d,%d,%d" % box, "--tracers-show", "--keys", keys] + SEEDS + [str(scn)],
                         capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    got = dumped_frames(run.stdout)
    assert len(got) == 8
    for f in range(8):
        assert got[f] == want[f], f
    assert b"38;2;" in want[0] and want[3] != want[2]      # yellow and blue escapes while it is shown
    # without --view the key does nothing; without --tracers-show the key turns it on
    run = subprocess.run([EXE, "--dump", "--frames", "3", "--window", "60x30", "--view", "%d,%d,%d,%d" % box, "--keys", "t"] + SEEDS + [str(scn)], capture_output=True, timeout=120)
    got = dumped_frames(run.stdout)
    assert run.returncode == 0 and b"38;2;" not in got[0] and b"38;2;" in got[1] and b"38;2;" in got[3]
    run = subprocess.run([EXE, "--dump", "--frames", "3", "--window", "60x30", "--keys", "t"] + SEEDS + [str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0 and b"38;2;" not in run.stdout


def test_usage_errors(scn):
    base = [EXE, "--dump", "--frames", "2"]
    bad = (["--tracer", "5"], ["--tracer", "5,6,7"], ["--tracer", "5,6x"], ["--tracer", "nan,6"], ["--tracer", "0.5,6"], ["--tracer", "5,39"], ["--tracer", "99,6"], ["--tracer", "5,-1"],
           ["--tracer-box", "1,1,4,4"], ["--tracer-box", "1,1,4,4:3"], ["--tracer-box", "1,1,4,4:2x"], ["--tracer-box", "0,1,4,4:2"], ["--tracer-box", "1,1,99,4:2"],
           ["--tracer-box", "1,1,4,39:1"], ["--tracer-box", "5,1,4,4:1"], ["--emit", "5"], ["--emit", "5,6:0"], ["--emit", "5,6:x"], ["--emit", "5,6:2:3"], ["--emit", "99,6"],
           ["--emit", "5,0.5:2"], ["--tracers-every", "0", "--tracers", "/dev/null"], ["--tracers-show"], ["--tracers-show", "--tracer", "5,6"],
           ["--tracer", "5,6"] * 1025, ["--tracer-box", "5,5,5,5:1"] * 65, ["--emit", "5,6"] * 65)
    for flags in bad:
        run = subprocess.run(base + flags + [str(scn)], capture_output=True, timeout=60)
        assert run.returncode == 1 and b"usage" in run.stderr and not run.stdout, flags[:4]
    run = subprocess.run(base + ["--tracer", "5,6"] * 1024 + ["--tracer-box", "5,5,5,5:1"] * 64 + ["--emit", "5,6"] * 64 + [str(scn)], capture_output=True, timeout=60)
    assert run.returncode == 0 and len(dumped_frames(run.stdout)) == 3
