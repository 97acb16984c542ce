"""The `euler` front end's run-long envelopes (docs/envelope.md): --envelope / --envelope-out / --envelope-ppm against a Python-driven handle doing the same, the
.f32 planes and the .ppm images byte for byte; the usage errors; --envelope beside --session-in; and a run without the new flags against the frames the handle
draws and against the run with them (the envelopes leave no trace in what the command writes)."""
import os
import subprocess

import numpy as np
import pytest

import euler_amd as ea
from golden_util import X, Y, load, scenario_text
from observer_util import EXE, dumped_frames

pytestmark = pytest.mark.gpu
SCALES = (1.0, 0.5, 12.0, 150.0)
CHANNELS = ((ea.ENV_ARRIVAL, "arrival"), (ea.ENV_WET, "wet"), (ea.ENV_SPEED, "speed"), (ea.ENV_PRESSURE, "pressure"))


@pytest.fixture
def scn(tmp_path):
    path = tmp_path / "block.txt"
    path.write_text(scenario_text(load("block_frames.npz")))
    return path


def test_planes_and_images_against_a_python_driven_handle(scn, tmp_path):
    sim = ea.Simulation(X, Y).load_text(scn.read_text())
    sim.set_envelope(ea.ENV_ALL)
    frames = [sim.draw(98, 38)]
    for _ in range(10):
        sim.step()
        frames.append(sim.draw(98, 38))
    px = sim.envelope_raster(None, X - 2, Y - 2)
    want = {name: (sim.envelope_field(c).tobytes(), b"P6\n%d %d\n255\n" % (X - 2, Y - 2) + ea.envelope_rgb(px, c, s).tobytes()) for (c, name), s in zip(CHANNELS, SCALES)}
    assert sim.envelope()[1] > 10 and len({v for v in want.values()}) == 4
    sim.close()
    out, img = str(tmp_path / "planes"), str(tmp_path / "a:b")      # (a colon in the prefix: the spec is cut at its last one)
    flags = ["--envelope", "all", "--envelope-out", out, "--envelope-ppm", img + ":" + ",".join("%g" % s for s in SCALES)]
    run = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "10"] + flags + [str(scn)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert dumped_frames(run.stdout) == frames
    for name, (plane, image) in want.items():
        assert open("%s.%s.f32" % (out, name), "rb").read() == plane, name
        assert open("%s.%s.ppm" % (img, name), "rb").read() == image, name
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]      # written under .tmp and renamed
    # only the enabled channels get a file
    out2 = str(tmp_path / "two")
    run2 = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "10", "--envelope", "wet,pressure", "--envelope-out", out2, str(scn)], capture_output=True, timeout=120)
    assert run2.returncode == 0 and sorted(f for f in os.listdir(tmp_path) if f.startswith("two.")) == ["two.pressure.f32", "two.wet.f32"]
    assert open(out2 + ".wet.f32", "rb").read() == want["wet"][0] and open(out2 + ".pressure.f32", "rb").read() == want["pressure"][0]
    # without any of the new flags every byte the command writes is what it was: the frames of a handle that never heard of envelopes, the same lines on stderr
    plain = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "10", str(scn)], capture_output=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout == run.stdout and plain.stderr == run.stderr
    bare = ea.Simulation(X, Y).load_text(scn.read_text())
    drawn = [bare.draw(98, 38)]
    for _ in range(10):
        bare.step()
        drawn.append(bare.draw(98, 38))
    bare.close()
    assert dumped_frames(plain.stdout) == drawn


def test_envelope_beside_session_in_starts_fresh_planes(scn, tmp_path):
    sess, out = str(tmp_path / "run.sess"), str(tmp_path / "late")
    first = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "4", "--envelope", "all", "--session-out", sess, str(scn)], capture_output=True, timeout=120)
    assert first.returncode == 0, first.stderr.decode()
    run = subprocess.run([EXE, "--dump", "--window", "98x38", "--frames", "8", "--session-in", sess, "--envelope", "arrival,wet", "--envelope-out", out], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    sim = ea.Simulation(X, Y)
    sim.load_session(sess, ignore_settings=True)      # (the command's handle and this one give the same bits: the test above)
    t0 = sim.time
    assert sim.envelope() == (0, 0) and t0 > 0      # the file carries no planes
    sim.set_envelope(ea.ENV_ARRIVAL | ea.ENV_WET)
    for _ in range(4):
        sim.step()
    arrival = sim.envelope_field(ea.ENV_ARRIVAL)
    assert open(out + ".arrival.f32", "rb").read() == arrival.tobytes() and open(out + ".wet.f32", "rb").read() == sim.envelope_field(ea.ENV_WET).tobytes()
    seen = arrival[arrival.view(np.uint32) != 0xFFFFFFFF]
    assert len(seen) and seen.min() > t0      # fresh planes: nothing arrived before the session's clock
    assert not os.path.exists(out + ".speed.f32")
    sim.close()


def test_usage_errors(scn, tmp_path):
    base = [EXE, "--dump", "--frames", "2"]
    p = str(tmp_path / "p")
    bad = (["--envelope", ""], ["--envelope", "wet,"], ["--envelope", ",wet"], ["--envelope", "Wet"], ["--envelope", "wets"], ["--envelope", "wet speed"], ["--envelope", "7"],
           ["--envelope-out", p], ["--envelope-ppm", p + ":1,1,1,1"], ["--envelope-out", p, "--envelope-ppm", p + ":1,1,1,1"],
           ["--envelope", "all", "--envelope-ppm", p], ["--envelope", "all", "--envelope-ppm", p + ":1,1,1"], ["--envelope", "all", "--envelope-ppm", p + ":1,1,1,1,1"],
           ["--envelope", "all", "--envelope-ppm", p + ":1,1,1,0"], ["--envelope", "all", "--envelope-ppm", p + ":1,-2,1,1"], ["--envelope", "all", "--envelope-ppm", p + ":1,1,nan,1"],
           ["--envelope", "all", "--envelope-ppm", p + ":1,1,1,1x"], ["--envelope", "all", "--envelope-ppm", ":1,1,1,1"])
    for flags in bad:
        run = subprocess.run(base + flags + [str(scn)], capture_output=True, timeout=60)
        assert run.returncode == 1 and b"usage" in run.stderr and not run.stdout, flags
    assert not os.listdir(tmp_path) or os.listdir(tmp_path) == ["block.txt"]
    # a file that cannot be written: status 1 behind the frames, and no .tmp is left
    run = subprocess.run(base + ["--envelope", "wet", "--envelope-out", str(tmp_path / "no-such-directory" / "x"), str(scn)], capture_output=True, timeout=60)
    assert run.returncode == 1 and b"--envelope-out: cannot write" in run.stderr and len(dumped_frames(run.stdout)) == 3
