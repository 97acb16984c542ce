"""The `euler` front end's scripted edits and brush keys (docs/editing.md): --edit against a Python-driven handle with the same edits, the brush of --view against
edit_box on the computed brush, the usage errors."""
import subprocess

import pytest

import euler_amd as ea
from golden_util import X, Y, load, scenario_text
from observer_util import EXE, dumped_frames

pytestmark = pytest.mark.gpu

BRUSH_KEYS = {"X": ea.EDIT_SOLID, "C": ea.EDIT_CLEAR, "S": ea.EDIT_SINK, "O": ea.EDIT_SOURCE, "W": ea.EDIT_FILL, "D": ea.EDIT_DRAIN}


def brush(box):
    """the viewed box shrunk about its centre: with Bw = x1 - x0 + 1, w = max(1, Bw / 4) cells from x0 + (Bw - w) / 2 on; the same in y"""
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    w, h = max(1, bw // 4), max(1, bh // 4)
    bx0, by0 = x0 + (bw - w) // 2, y0 + (bh - h) // 2
    return bx0, by0, bx0 + w - 1, by0 + h - 1


@pytest.fixture
def scn(tmp_path):
    path = tmp_path / "block.txt"
    path.write_text(scenario_text(load("block_frames.npz")))
    return path


def test_scripted_edits(scn):
    """--edit F:OP:BOX is applied right before the step that produces frame F, in command-line order; F = 0 before frame 0 is drawn"""
    edits = [(5, "solid", (30, 3, 33, 20)), (5, "fill", (70, 20, 80, 30)), (0, "drain", (10, 15, 20, 25)), (9, "source", (60, 33, 63, 35)), (9, "clear", (30, 3, 33, 8)),
             (11, "sink", (40, 1, 50, 2))]
    ops = {"solid": ea.EDIT_SOLID, "clear": ea.EDIT_CLEAR, "sink": ea.EDIT_SINK, "source": ea.EDIT_SOURCE, "fill": ea.EDIT_FILL, "drain": ea.EDIT_DRAIN}
    sim = ea.Simulation(X, Y).load_text(scn.read_text())
    plain, fitted, viewed = [], [], []
    vbox = (20, 2, 68, 30)
    for f in range(13):
        if f:
            for (fr, name, box) in edits:
                if fr == f:
                    sim.edit_box(ops[name], box)
            sim.step()
        else:
            for (fr, name, box) in edits:
                if fr == 0:
                    sim.edit_box(ops[name], box)
        plain.append(sim.draw(98, 38)); fitted.append(sim.render_fit(40, 15)); viewed.append(sim.render_view(vbox, 98, 38))
    markers = sim.stats().n_markers
    sim.close()
    assert len(set(plain)) >= 10      # (the scene moves)
    flags = []
    for (fr, name, box) in edits:
        flags += ["--edit", "%d:%s:%d,%d,%d,%d" % ((fr, name) + box)]
    base = [EXE, "--dump", "--frames", "12"]
    for extra, want in ((["--window", "98x38"], plain), (["--window", "40x15", "--fit"], fitted), (["--window", "98x38", "--view", "%d,%d,%d,%d" % vbox], viewed)):
        run = subprocess.run(base + extra + flags + [str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0, run.stderr.decode()
        got = dumped_frames(run.stdout)
        assert len(got) == 13
        for f in range(13):
            assert got[f] == want[f], (extra, f)
        assert ("markers %d" % markers) in run.stderr.decode()
    # without the edits: other frames
    run = subprocess.run(base + ["--window", "98x38", str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0 and dumped_frames(run.stdout) != plain


def test_brush_keys(scn):
    """--view --keys '....W..X': the brush formula on the box as the pan and zoom keys left it; without --view the capitals do nothing"""
    start = (10, 5, 58, 23)
    import viewport_ref as vref
    for keys in ("....W..X", "l+W-DkOhSC"):
        sim = ea.Simulation(X, Y).load_text(scn.read_text())
        box, want, brushes = start, [], []
        n = len(keys) + 2
        for f in range(n + 1):
            if f:
                key = keys[f - 1] if f - 1 < len(keys) else "."
                if key in BRUSH_KEYS:
                    brushes.append(brush(box))
                    sim.edit_box(BRUSH_KEYS[key], brushes[-1])
                else:
                    box = vref.view_key(box, key, X - 2, Y - 2)
                sim.step()
            want.append(sim.render_view(box, 98, 38))
        sim.close()
        if keys == "....W..X":
            assert brushes == [(28, 12, 39, 15)] * 2      # Bw = 49, Bh = 19: w = 12 from 10 + 18, h = 4 from 5 + 7
        base = [EXE, "--dump", "--window", "98x38", "--frames", str(n), "--keys", keys]
        run = subprocess.run(base + ["--view", "%d,%d,%d,%d" % start, str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0, run.stderr.decode()
        got = dumped_frames(run.stdout)
        assert len(got) == n + 1
        for f in range(n + 1):
            assert got[f] == want[f], (keys, f)
        run = subprocess.run(base + [str(scn)], capture_output=True, timeout=120)
        plain = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", str(n), str(scn)], capture_output=True, timeout=120)
        assert run.returncode == 0 and plain.returncode == 0 and run.stdout == plain.stdout


def test_usage_errors(scn):
    base = [EXE, "--dump", "--frames", "2"]
    bad = (["--edit", "5:solid:0,1,10,10"], ["--edit", "5:solid:1,1,99,10"], ["--edit", "5:solid:1,1,10,39"], ["--edit", "5:solid:5,1,4,10"], ["--edit", "5:wall:1,1,4,10"],
           ["--edit", "5:solid:1,1,4"], ["--edit", "5:solid:1,1,4,10x"], ["--edit", "-1:solid:1,1,4,10"], ["--edit", "solid:1,1,4,10"], ["--edit", "5:SOLID:1,1,4,10"],
           ["--edit"], ["--edit", "1:fill:1,1,2,2"] * 65)
    for flags in bad:
        run = subprocess.run(base + flags + [str(scn)], capture_output=True, timeout=60)
        assert run.returncode == 1 and b"usage" in run.stderr and not run.stdout, flags
    run = subprocess.run(base + ["--edit", "1:fill:1,1,2,2"] * 64 + [str(scn)], capture_output=True, timeout=60)
    assert run.returncode == 0 and len(dumped_frames(run.stdout)) == 3
