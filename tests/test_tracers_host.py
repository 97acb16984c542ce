"""The host half of the passive tracers (docs/tracers.md), no GPU: the layout of the record from a small C program, the host C code under the sanitizers
(tests/c/sanitize_tracers.c), the painter and the pixel-of-a-cell formula against brute force, the one-marker walk of tests/tracers_ref.py against the
oracle's own eo_advect_markers, the preconditions the GPU tests (tests/test_gpu_tracers.py) rely on, checked here on the oracle, and a known answer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import tracers_ref as tref
from euler_amd import scenarios
from golden_util import X, Y, load, scenario_text
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return tref.build(tmp_path_factory.mktemp("tracers"))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ----------------------------------------------------------------------------- layout, sanitizers
@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_layout(tmp_path):
    t, p = ea.TRACER_DTYPE, ea.OVERVIEW_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n'
                   '  printf("%zu %zu %u %d %d %d %d %d %d %d", sizeof(euler_tracer), sizeof(euler_overview_px), (unsigned)EULER_TRACERS_MAX, EULER_TRACER_WET, EULER_TRACER_RETIRED,\n'
                   '         EULER_TRACER_IN_SOLID, EULER_TRACER_IN_SINK, EULER_TRACER_LOST, EULER_TRACER_WAS_DRY, EULER_TRACER_RASTER_ALL);\n'
                   + "".join('  printf(" %%zu", offsetof(euler_tracer, %s));\n' % n for n in t.names)
                   + "".join('  printf(" %%zu", offsetof(euler_overview_px, %s));\n' % n for n in p.names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[:3] == [32, 48, 1 << 22] == [t.itemsize, p.itemsize, ea.TRACERS_MAX]
    assert out[3:10] == [1, 2, 4, 8, 16, 32, 1] == [ea.TRACER_WET, ea.TRACER_RETIRED, ea.TRACER_IN_SOLID, ea.TRACER_IN_SINK, ea.TRACER_LOST, ea.TRACER_WAS_DRY, ea.TRACER_RASTER_ALL]
    assert out[10:18] == [t.fields[n][1] for n in t.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert out[18:] == [p.fields[n][1] for n in p.names]
    assert [t.fields[n][0] for n in t.names] == [np.float32] * 5 + [np.uint32] * 3


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the checker with every refusal and their order, the lattice, the pixel of a cell, the painter and the command's three spec parsers"""
    exe = str(tmp_path / "sanitize_tracers")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_tracers.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- the pixel of a cell, the raster's restatement, the painter, the lattice
def test_pixel_formula_against_the_covering_definition():
    for B in range(1, 41):
        for W in range(1, B + 1):
            want = [tref.pixel_brute(c, B, W) for c in range(B)]
            assert list(tref.pixel(np.arange(B), B, W)) == want, (B, W)
            assert want[0] == 0 and want[-1] == W - 1 and sorted(set(want)) == list(range(W))      # every pixel covers a cell: none is empty


def test_raster_restatement_against_brute_force():
    rng = np.random.default_rng(5)
    Xg, Yg = 47, 31
    xy = np.stack([rng.uniform(1, Xg - 1, 400), rng.uniform(1, Yg - 1, 400)], 1).astype(F32)
    xy[:4] = [[7.0, 5.0], [12.0, 9.999999], [np.nan, 5.0], [np.inf, 5.0]]      # on the box's edges; counted nowhere
    rec = tref.records(xy)
    rec["flags"][::7] |= ea.TRACER_RETIRED
    for box in ((1, 1, Xg - 2, Yg - 2), (7, 5, 12, 9), (7, 5, 7, 5), (3, 2, 40, 25)):
        x0, y0, x1, y1 = box
        Bw, Bh = x1 - x0 + 1, y1 - y0 + 1
        for W, H in ((Bw, Bh), (1, 1), (max(Bw // 2, 1), max(Bh // 3, 1)), (max(Bw - 1, 1), max(Bh - 1, 1))):
            for every in (False, True):
                want = np.zeros((H, W), np.uint32)
                for r in rec:
                    if not (np.isfinite(r["x"]) and np.isfinite(r["y"])) or ((r["flags"] & ea.TRACER_RETIRED) and not every):
                        continue
                    cx, cy = int(np.floor(r["x"])), int(np.floor(r["y"]))
                    if x0 <= cx <= x1 and y0 <= cy <= y1:
                        want[tref.pixel_brute(y1 - cy, Bh, H), tref.pixel_brute(cx - x0, Bw, W)] += 1
                assert np.array_equal(tref.raster(rec, box, W, H, every), want), (box, W, H, every)


def test_painter_against_numpy():
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (5, 7), (16, 9)):
        px = np.zeros((h, w), ea.OVERVIEW_DTYPE)
        px["cells"] = 16
        px["water"] = rng.integers(0, 17, (h, w)) * (rng.random((h, w)) < 0.7)
        px["marks"] = rng.integers(0, 40, (h, w))
        px["dye"] = rng.integers(0, 1 << 40, (h, w, 3))
        counts = (rng.integers(0, 4, (h, w)) * (rng.random((h, w)) < 0.5)).astype(np.uint32)
        for fg, bg in (((1, 0.9, 0), (0.25, 0.5, 1)), ((1, 0.9, 0), None), ((0.3, np.nan, 2.0), (-1.0, 0.123456, 1.0))):
            got = ea.tracer_paint(counts, px, fg, bg)
            want = tref.paint(counts, px, fg, bg)
            assert got.tobytes() == want.tobytes(), (h, w, fg, bg)
            dry = px["water"] == 0
            assert got[dry].tobytes() == px[dry].tobytes()
            if bg is None:
                keep = counts == 0
                assert got[keep].tobytes() == px[keep].tobytes()
    with pytest.raises(ValueError):
        ea.tracer_paint(np.zeros((2, 3), np.uint32), np.zeros((3, 2), ea.OVERVIEW_DTYPE), (1, 1, 1))


def test_lattice_binding():
    for k in (1, 2, 4):
        xy = ea.tracer_lattice((3, 5, 4, 7), k)
        want = [(x + (i + 0.5) / k, y + (j + 0.5) / k) for x in (3, 4) for y in (5, 6, 7) for i in range(k) for j in range(k)]
        assert xy.dtype == F32 and xy.shape == (6 * k * k, 2) and np.array_equal(xy, np.array(want, F32))
    for bad in ((3, 5, 2, 7, 2), (3, 5, 4, 7, 3)):
        with pytest.raises(ValueError):
            ea.tracer_lattice(bad[:4], bad[4])


# ----------------------------------------------------------------------------- the one-marker walk
def test_one_marker_walk_is_the_oracles_without_the_midpoint(libs):
    """rk2 = 0: a tracer's walk equals eo_advect_markers on an array of that one marker, bit for bit; the oracle's own markers stay as they were"""
    am, tw = libs
    o = Oracle(X, Y).load_text(scenario_text(load("waterfall_frames.npz")))
    for _ in range(6):
        o.step()
    rng = np.random.default_rng(3)
    pick = rng.choice(o.n_markers, 60, replace=False)
    xy = np.concatenate([o.markers[pick], [[50.5, 35.5], [2.25, 2.75]]]).astype(F32)
    dt = o.timestep(0.1)
    keep = o.markers.copy()
    got = tref.walk(tw, o, xy, dt, False)
    assert np.array_equal(bits(o.markers), bits(keep)) and o.n_markers == len(keep)
    moved = 0
    for k, p in enumerate(xy):
        o.set_markers(p[None])
        o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
        assert np.array_equal(bits(o.markers[0]), bits(got[k])), k
        moved += not np.array_equal(bits(p), bits(got[k]))
        o.set_markers(keep)
    assert moved > 30
    # several tracers in ONE marker array would be coupled by the dt chain; the walk never does that: any order, any subset, the same bits
    perm = rng.permutation(len(xy))
    assert np.array_equal(bits(tref.walk(tw, o, xy[perm], dt, False)), bits(got[perm]))
    assert np.array_equal(bits(tref.walk(tw, o, xy[:1], dt, True)), bits(tref.walk(tw, o, xy, dt, True)[:1]))


# ----------------------------------------------------------------------------- what the GPU tests rely on, checked on the oracle
def test_gpu_test_preconditions(libs):
    import test_gpu_tracers as g      # (importing it needs no GPU)
    am, tw = libs
    # the tracked-marker scene keeps its marker count constant over its frames (no source, no sink reached): markers[0] is never moved by a deletion
    o = g.tracked_scene_oracle()
    n0 = o.n_markers
    assert n0 > 0
    for _ in range(g.TRACKED_FRAMES):
        tref.step(libs, o, tref.records(np.zeros((0, 2))))
        assert o.n_markers == n0
    # the free runs' script: a wall is raised over live tracers, some retire in it and some in the sink, some walks hit a wall, some tracers are dry for part of the run
    for mode in ("rk1", "maccormack+rk2"):
        hit = walled = 0
        for ev in g.free_run_script(libs, (X, Y), mode):
            if ev[0] == "wall":
                walled = int((((rec["flags"] & ea.TRACER_RETIRED) == 0) & g.in_box(rec, ev[1])).sum())      # (rec: the records after the frame before)
            elif ev[0] == "frame":
                rec = ev[2]
                live = (rec["flags"] & ea.TRACER_RETIRED) == 0
                # a walk that hits a wall leaves its tracer on the edge of the cell it stopped in
                hit += int((live & (rec["x"] == np.floor(rec["x"]))).sum() + (live & (rec["y"] == np.floor(rec["y"]))).sum())
        fl = rec["flags"]
        assert walled >= 1, mode
        assert ((fl & ea.TRACER_IN_SOLID) != 0).sum() >= 1 + walled and ((fl & ea.TRACER_IN_SINK) != 0).sum() >= 1, mode
        part = (rec["wet_time"] > 0) & ((fl & ea.TRACER_WAS_DRY) != 0)
        assert part.sum() >= 1 and ((fl & ea.TRACER_WAS_DRY) == 0).sum() >= 1, mode
        assert (rec["substeps"] > 20).sum() > 10 and hit >= 1, mode


# ----------------------------------------------------------------------------- a known answer
def test_tracer_in_air_over_a_tank_at_rest(libs):
    """a half tank at rest: nothing moves; a tracer in the air keeps its position, path == 0, age is the float sum of the dts, it was never wet; one in the
    water keeps its position too, wet all the time"""
    o = Oracle(70, 40).load_half_tank()
    rec = tref.records([[30.5, 30.25], [30.5, 8.25]])
    age = F32(0)
    clock = 0.0
    for _ in range(3):
        ft = F32(0.1)
        n = 0
        while ft > 0 and n < 8:
            dt = F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
            ft = F32(ft - dt)
            tref.substep(libs, o, rec, float(dt))
            age = F32(age + dt)
            clock += float(dt)
            n += 1
    assert bits(rec["x"][:1]) == bits([30.5]) and bits(rec["y"][:1]) == bits([30.25])
    assert rec["path"][0] == 0.0 and rec["substeps"][0] == rec["substeps"][1] > 0
    assert np.array_equal(bits(rec["age"]), bits([age, age]))
    assert rec["wet_time"][0] == 0 and bits(rec["wet_time"][1:]) == bits([age])
    assert rec["flags"].tolist() == [ea.TRACER_WAS_DRY, ea.TRACER_WET]
    o2 = Oracle(70, 40).load_half_tank()
    assert tref.step(libs, o2, tref.records([[30.5, 30.25]])) > 0.0
