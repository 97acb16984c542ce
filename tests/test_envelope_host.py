"""The run-long envelopes without a GPU (docs/envelope.md): the two restatements of tests/envelope_ref.py against each other on random scenes, the record's layout
from a small C program, the host C code under the sanitizers (tests/c/sanitize_envelope.c), the raster's pixel formula against brute force, a known answer on the
CPU composition - a half tank at rest -, and the preconditions of the GPU scenes (test_gpu_envelope.py), checked on the oracle so that the GPU tests cannot pass
vacuously.  The scenes and the oracle runs are shared with the GPU tests: each run is made once per process."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import edit_ref as eref
import envelope_ref as er
import euler_amd as ea
import forcing_ref as fref
import heat_ref as href
from euler_amd import scenarios
from golden_util import load, scenario_text
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 20
EDIT_FRAME = 8
TRANSPORTS = ((0, 0), (1, 0), (1, 1))      # (rk2, maccormack): RK1, RK2, MacCormack + RK2
FORCING = fref.forcing((3.0, -8.0), (1.5, 0.5, 0.8, 0.3))
HEAT = href.heat(2.0, 3.0, 0.3, 1.0)      # ambient, beta, kappa, source_t: a strong buoyancy
HEAT_BOXES = [(href.RATE, 30.0, (10, 3, 30, 12)), (href.FIX, 4.0, (36, 4, 60, 20))]


# ----------------------------------------------------------------------------- the scenes of the GPU tests
def flume_text():
    from test_gpu_tracers import flume_text as text      # (the flume of the tracer tests)
    return text()


@functools.lru_cache(maxsize=None)
def scene(name):
    """(X, Y), text, upscale"""
    if name == "waterfall":      # the reference's, from tests/golden/: 100 x 40, four cells per lane, one band
        return (100, 40), scenario_text(load("waterfall_frames.npz")), False
    if name == "flume":          # 103 x 41: the one-cell-per-lane path
        return (103, 41), flume_text(), True
    if name == "dam":            # 264 x 136: 5 x 3 tiles, ragged in both directions, most of them dry at frame 0
        return (264, 136), scenarios.dam_break(), True
    if name == "wide":           # the flume's picture on the same grid: its front crosses x = 128 into a tile that held no water at frame 0
        return (264, 136), flume_text(), True
    raise KeyError(name)


SCENES = ("waterfall", "flume", "dam", "wide")
WALL_BOX = (4, 1, 12, 134)      # of the wide flume: the cells beside its left wall, floor to ceiling
PRESSURE_PEAKS_AT_FRAME_ENDS =("waterfall", "dam")      # free runs in which a look per frame misses no pressure peak (test_free_runs_are_not_trivial); the flumes' do


def solid_edit(o, wall):
    """EULER_EDIT_SOLID on the oracle: the masks, the markers inside deleted in the reference's order, the counts"""
    sl = (slice(wall[1], wall[3] + 1), slice(wall[0], wall[2] + 1))
    o.solid[sl], o.source[sl], o.sink[sl] = 1, 0, 0
    o.set_markers(eref.delete_in_box_vectorised(o.markers, wall))
    o.count[sl] = 0


def edit_wall(name, count):
    """3 x 3 cells in the water of the scene as it stands: the wet cells nearest their centroid"""
    ys, xs = np.nonzero(count[2:-2, 2:-2])
    k = np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2)
    x, y = int(xs[k]) + 2, int(ys[k]) + 2
    return (x - 1, y - 1, x + 1, y + 1)


def acc_at(f, t):
    """the uniform acceleration as the library itself forms it (host only): no libm difference reaches the comparison with the device"""
    return ea.forcing_at(ea.forcing_record((f["gx"], f["gy"]), (f["shake_x"], f["shake_y"], f["shake_hz"], f["shake_phase"]), 0), t)


class Run:
    """what an oracle run leaves: the envelope at substep rate, the one a caller would gather by looking once per frame, the (t, dt) of every substep,
    the tiles that were dry at frame 0, the wall of the edit and the words its cells held when it was raised"""


@functools.lru_cache(maxsize=None)
def oracle_run(am, name, rk2=0, mc=0, edit=False, forced=False, heated=False, frames=FRAMES):
    size, text, up = scene(name)
    o = Oracle(*size).load_text(text, upscale=up)
    T = href.field(o, HEAT) if heated else None
    r = Run()
    r.env, r.per_frame, r.substeps, r.wall, r.at_edit = er.Envelope(*size), er.Envelope(*size), [], None, None
    r.count0 = np.array(o.count)
    clock = fref.Clock()

    def fold_frame():      # behind the last substep of a frame: what a look per frame sees
        t, dt = r.substeps[-1]
        er.fold(r.per_frame, o, t, dt)

    for f in range(frames):
        if edit and f == EDIT_FRAME:
            r.wall = edit_wall(name, np.array(o.count))
            r.wet_before = np.array(o.count)[r.wall[1]:r.wall[3] + 1, r.wall[0]:r.wall[2] + 1] != 0
            solid_edit(o, r.wall)
            r.at_edit = r.env.copy()
        n_before = len(r.substeps)
        t0 = clock.t
        ft = er.F32(0.1)
        n = 0
        while ft > 0 and n < 8:
            dt = er.F32(o.lib.eo_calculate_timestep(o.ptr, C.c_float(ft)))
            ft = er.F32(ft - dt)
            r.substeps.append((clock.t, float(dt)))
            if heated:      # heat_ref's composition of the same stages with the temperature in two of them, then the update from what it leaves
                href.substep(am, o, T, HEAT, HEAT_BOXES, float(dt), None, (), clock, rk2, mc)
                er.fold(r.env, o, *r.substeps[-1])
            else:
                er.substep(am, o, r.env, float(dt), clock, FORCING if forced else None, (), rk2, mc, acc_at if forced else None)
            n += 1
        o.c.last_substeps = n
        o.c.frame_count += 1
        fold_frame()
        assert len(r.substeps) > n_before and clock.t > t0
    r.t_final = clock.t
    r.solid, r.count, r.u = np.array(o.solid), np.array(o.count), np.array(o.u)
    o.close()
    return r


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("envelope_host"))


# ----------------------------------------------------------------------------- the restatements against each other
def random_state(rng, X, Y):
    solid = (rng.random((Y, X)) < 0.15).astype(np.uint8)
    solid[0, :] = solid[-1, :] = solid[:, 0] = solid[:, -1] = 1
    count = (rng.integers(0, 4, (Y, X)) * (rng.random((Y, X)) < 0.6)).astype(np.uint8)
    count[0, 3] = count[2, 0] = 2      # markers on the border: not interior, never recorded
    solid[0, 3] = solid[2, 0] = 0
    u = (rng.standard_normal((Y, X)) * 3).astype(np.float32)
    v = (rng.standard_normal((Y, X)) * 3).astype(np.float32)
    p = rng.standard_normal((Y, X)) * 40 + 20
    for a, vals in ((u, (np.nan, np.inf, -0.0)), (v, (np.nan, -np.inf, 1e30)), (p, (np.nan, np.inf, -np.inf, -0.0, 1e300, 1e-300))):
        for val in vals:
            a[rng.integers(1, Y - 1), rng.integers(1, X - 1)] = val
    return solid, count, u, v, p


def assert_planes(got, want, what):
    assert got.channels == want.channels and set(got.planes) == set(want.planes), what
    for c in want.planes:
        bad = np.argwhere(got.planes[c] != want.planes[c])
        assert not len(bad), "%s: %s plane at (x, y) = (%d, %d): 0x%08x, expected 0x%08x (%d cells differ)" % (
            what, er.NAMES[c], bad[0][1], bad[0][0], got.planes[c][tuple(bad[0])], want.planes[c][tuple(bad[0])], len(bad))


@pytest.mark.parametrize("size", [(17, 9), (24, 13)])
@pytest.mark.parametrize("channels", [er.ALL, er.ARRIVAL | er.WET, er.SPEED, er.PRESSURE])
def test_numpy_and_loop_updates_agree(size, channels):
    rng = np.random.default_rng(size[0] * 100 + channels)
    a, b = er.Envelope(*size, channels), er.Envelope(*size, channels)
    t = 0.0
    for k in range(6):
        g = random_state(rng, *size)
        dt = float(np.float32(rng.uniform(1e-3, 0.1)))
        er.update(a, *g, t, dt)
        er.update_loop(b, *g, t, dt)
        assert_planes(a, b, "substep %d" % k)
        t += dt
    assert a.substeps == b.substeps == 6
    if channels & er.ARRIVAL:      # both kinds of word occur, and a cell wetted later arrived later
        arr = a.planes[er.ARRIVAL]
        assert (arr == er.NEVER).any() and len(np.unique(arr[arr != er.NEVER])) > 1
        assert (arr[0, :] == er.NEVER).all() and (arr[:, 0] == er.NEVER).all()
    if channels & er.PRESSURE:
        assert np.isfinite(a.f(er.PRESSURE)[a.f(er.PRESSURE) < np.inf]).all() and not np.isnan(a.f(er.PRESSURE)).any() and (a.planes[er.PRESSURE] < 0x80000000).all()


def test_update_rules_on_planted_values():
    X, Y = 8, 6
    solid, count = np.zeros((Y, X), np.uint8), np.zeros((Y, X), np.uint8)
    u, v, p = np.zeros((Y, X), np.float32), np.zeros((Y, X), np.float32), np.zeros((Y, X))
    count[2, 2:6] = 1
    u[2, 2], u[2, 1], v[2, 2], v[1, 2] = 3.0, 1.0, 2.0, 6.0      # dx = 2, dy = 4: s2 = 20
    p[2, 2:6] = [12.5, -3.0, np.nan, 1e300]
    e = er.Envelope(X, Y)
    er.update(e, solid, count, u, v, p, 1.0, 0.25)
    assert e.f(er.ARRIVAL)[2, 2] == np.float32(1.25) and e.planes[er.ARRIVAL][3, 2] == er.NEVER
    assert e.f(er.WET)[2, 2] == np.float32(0.25) and e.f(er.SPEED)[2, 2] == np.float32(20.0)
    assert list(e.f(er.PRESSURE)[2, 2:6]) == [12.5, 0.0, 0.0, np.inf]
    solid[2, 2] = 1      # solid now, wet earlier: the words stay
    count[2, 6] = 3
    p[2, 3] = 4.0
    er.update(e, solid, count, u, v, p, 1.25, 0.5)
    assert e.f(er.ARRIVAL)[2, 2] == np.float32(1.25) and e.f(er.WET)[2, 2] == np.float32(0.25) and e.f(er.PRESSURE)[2, 2] == 12.5
    assert e.f(er.ARRIVAL)[2, 3] == np.float32(1.25) and e.f(er.ARRIVAL)[2, 6] == np.float32(1.75)
    assert e.f(er.WET)[2, 3] == np.float32(0.75) and e.f(er.PRESSURE)[2, 3] == 4.0 and e.substeps == 2


def test_raster_numpy_against_loop_and_brute_force():
    """every 1 <= W <= Bw <= 40: the pixel a cell falls in by the loop's formula is the pixel whose range of the overview's geometry holds it"""
    for Bw in range(1, 41):
        for W in range(1, Bw + 1):
            edges = er.pixel_edges(3, Bw, W)
            assert edges[0] == 3 and edges[-1] == 3 + Bw and all(b > a for a, b in zip(edges, edges[1:]))
            for x in range(3, 3 + Bw):
                px = ((x - 3 + 1) * W - 1) // Bw
                assert edges[px] <= x < edges[px + 1], (Bw, W, x)
            rows = er.pixel_rows(5, 5 + Bw - 1, W)
            assert rows[0][0] == 5 + Bw - 1 and rows[-1][1] == 5
            for y in range(5, 5 + Bw):
                py = ((5 + Bw - 1 - y + 1) * W - 1) // Bw
                assert rows[py][1] <= y <= rows[py][0], (Bw, W, y)
    rng = np.random.default_rng(11)
    X, Y = 47, 29
    for channels in (er.ALL, er.WET | er.PRESSURE, er.ARRIVAL, 0):
        e = er.Envelope(X, Y, channels)
        for c, pl in e.planes.items():
            pl[...] = rng.random((Y, X)).astype(np.float32).view(np.uint32)
            pl[rng.random((Y, X)) < 0.5] = er.NEVER if c == er.ARRIVAL else 0
        for _ in range(12):
            x0, y0 = int(rng.integers(1, X - 2)), int(rng.integers(1, Y - 2))
            x1, y1 = int(rng.integers(x0, X - 1)), int(rng.integers(y0, Y - 1))
            W, H = int(rng.integers(1, x1 - x0 + 2)), int(rng.integers(1, y1 - y0 + 2))
            a, b = er.raster(e, (x0, y0, x1, y1), W, H), er.raster_loop(e, (x0, y0, x1, y1), W, H)
            assert a.tobytes() == b.tobytes(), (channels, x0, y0, x1, y1, W, H)
            assert int(a["cells"].sum()) == (x1 - x0 + 1) * (y1 - y0 + 1)
            if not channels & er.ARRIVAL:
                assert not a["touched"].any() and (a["arrival_min"] == er.NEVER).all() and not a["arrival_max"].any()


def random_records(rng, shape):
    px = np.zeros(shape, er.PX_DTYPE)
    for n in ("arrival_min", "arrival_max", "wet_max", "speed2_max", "p_max"):
        px[n] = (rng.random(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32).view(np.uint32)
    px["touched"] = rng.integers(0, 3, shape)
    px["cells"] = px["touched"] + 1
    dry = px["touched"] == 0
    px["arrival_min"][dry], px["arrival_max"][dry] = er.NEVER, 0
    for n in ("wet_max", "speed2_max", "p_max"):      # (with touched == 0: the black pixels of the other channels)
        px[n][rng.random(shape) < 0.3] = 0
    px["wet_max"].flat[0] = np.array(np.inf, np.float32).view(np.uint32)
    px["speed2_max"].flat[1] = np.array(np.nan, np.float32).view(np.uint32)
    return px


def test_rgb_against_both_restatements():
    rng = np.random.default_rng(3)
    px = random_records(rng, (9, 14))
    for c, scale in ((er.ARRIVAL, 2.0), (er.WET, 0.5), (er.SPEED, 7.0), (er.PRESSURE, 100.0), (er.PRESSURE, 1e-3)):
        got = ea.envelope_rgb(px, c, scale)
        assert got.tobytes() == er.rgb(px, c, scale).tobytes() == er.rgb_loop(px, c, scale).tobytes(), c
        assert (got[..., 0] == 255).any() and (got.reshape(-1, 3).sum(1) == 0).any()
    for bad in (0, 3, 15, 16):
        with pytest.raises(ea.EulerError):
            ea.envelope_rgb(px, bad, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ea.EulerError):
            ea.envelope_rgb(px, er.WET, bad)


def test_python_constants_and_dtype_mirror_the_header():
    import re
    hdr = open(os.path.join(ROOT, "include", "euler.h")).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(EULER_ENV_[A-Z]+)\s*=\s*(\d+)", hdr)}
    assert values == {"EULER_ENV_ARRIVAL": ea.ENV_ARRIVAL, "EULER_ENV_WET": ea.ENV_WET, "EULER_ENV_SPEED": ea.ENV_SPEED, "EULER_ENV_PRESSURE": ea.ENV_PRESSURE, "EULER_ENV_ALL": ea.ENV_ALL}
    assert (er.ARRIVAL, er.WET, er.SPEED, er.PRESSURE, er.ALL) == (ea.ENV_ARRIVAL, ea.ENV_WET, ea.ENV_SPEED, ea.ENV_PRESSURE, ea.ENV_ALL)
    assert ea.ENVELOPE_PX_DTYPE == er.PX_DTYPE


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_record_layout_from_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\n'
                   'int main(void) { printf("%zu", sizeof(euler_envelope_px));\n'
                   + "".join('printf(" %%zu", offsetof(euler_envelope_px, %s));\n' % n for n in er.PX_DTYPE.names) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    out = [int(t) for t in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert out == [32] + [er.PX_DTYPE.fields[n][1] for n in er.PX_DTYPE.names] == [32, 0, 4, 8, 12, 16, 20, 24, 28]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the word checker of euler_envelope_set_field, euler_envelope_rgb and the command's parsers and writer"""
    exe = str(tmp_path / "sanitize_envelope")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_envelope.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- a known answer: a half tank at rest
HYDROSTATIC_REL = 1e-4      # the margin of test_gauges_host.hydrostatic_bound: quantisation of 2^-8 against pressures of at least 10 and a solver tolerance of 1e-6


@pytest.mark.parametrize("size", [(64, 40), (100, 70)])
def test_half_tank_at_rest_known_answer(size):
    Xg, Yg = size
    o = Oracle(Xg, Yg).load_half_tank()
    fluid0 = er.fluid_cells(o.solid, o.count)
    env, clock = er.Envelope(Xg, Yg), fref.Clock()
    dts = []
    for left in (0.1, 0.07, 0.1, 0.033, 0.1):      # the frame time left cuts some of the steps short: the sum below is of unequal terms
        dt = o.timestep(left)
        er.substep(None, o, env, dt, clock)
        dts.append(np.float32(dt))
        assert o.c.last_pcg_iterations < 100      # under the cap: the solve converged
    assert len(set(dts)) > 1
    fluid = er.fluid_cells(o.solid, o.count)
    assert fluid.any() and (fluid == fluid0).all()      # at rest: no cell wets or dries
    first = np.float32(np.float64(0.0) + np.float64(dts[0]))
    wet = np.float32(0)
    for dt in dts:
        wet = np.float32(wet + dt)
    assert (env.f(er.ARRIVAL)[fluid] == first).all() and (env.f(er.WET)[fluid] == wet).all()
    assert (env.planes[er.ARRIVAL][~fluid] == er.NEVER).all()
    for c in (er.WET, er.SPEED, er.PRESSURE):
        assert not env.planes[c][~fluid].any(), er.NAMES[c]
    # the k-th fluid cell from the top of a column carries 10 k, within the gauges' margin
    worst = 0.0
    depth = 0
    for x in range(1, Xg - 1):
        ys = np.flatnonzero(fluid[:, x])[::-1]
        assert (np.diff(ys) == -1).all()      # (a column of the tank's wall holds none)
        depth = max(depth, len(ys))
        for k, y in enumerate(ys, 1):
            err = abs(float(env.f(er.PRESSURE)[y, x]) - 10.0 * k)
            worst = max(worst, err / (10.0 * k))
            assert err <= HYDROSTATIC_REL * 10.0 * k, (x, y, k, env.f(er.PRESSURE)[y, x])
    # at rest the speed is 0 up to what that margin lets through: per substep a face moves by at most dt times the error of the two pressures beside it
    assert depth >= 5 and fluid.sum() >= depth * (Xg - 8)
    v_bound = sum(float(dt) for dt in dts) * 2 * HYDROSTATIC_REL * 10.0 * depth
    print("worst relative pressure error %.3g; largest speed^2 %.3g, bound %.3g" % (worst, env.f(er.SPEED).max(), 2 * v_bound ** 2))
    assert env.f(er.SPEED).max() <= 2 * v_bound ** 2


# ----------------------------------------------------------------------------- the preconditions of the GPU scenes
@pytest.mark.parametrize("name", SCENES)
def test_free_runs_are_not_trivial(am, name):
    r = oracle_run(am, name)
    env = r.env
    arr, wet = env.f(er.ARRIVAL).astype(np.float64), env.f(er.WET).astype(np.float64)
    hit = env.planes[er.ARRIVAL] != er.NEVER
    assert hit.any() and (~hit[1:-1, 1:-1]).any()      # the water reached some cells and not others
    assert len(np.unique(env.planes[er.ARRIVAL][hit])) > 20      # fronts moved: many arrival times
    assert env.substeps == len(r.substeps) > FRAMES      # several substeps to a frame
    # some cell dried again: a cell that stayed wet from its arrival on holds the float sum of the dts from that substep on, in order; one that dried holds less
    dried, stayed = np.zeros(hit.shape, bool), np.zeros(hit.shape, bool)
    for k, (t, dt) in enumerate(r.substeps):
        full = np.float32(0)
        for (_, d) in r.substeps[k:]:
            full = np.float32(full + np.float32(d))
        here = hit & (env.f(er.ARRIVAL) == er.t_end_of(t, dt))
        assert (env.f(er.WET)[here] <= full).all()
        dried |= here & (env.f(er.WET) < full)
        stayed |= here & (env.f(er.WET) == full)
    assert ((dried | stayed) == hit).all() and stayed.any() and (wet[dried] < (r.t_final - arr)[dried] + 0.1).all()
    print("%s: %d cells reached, %d dried again, %d substeps" % (name, hit.sum(), dried.sum(), env.substeps))
    assert dried.any()
    # sampling once per frame would miss peaks: some cell's peak speed - in the flume, where the collapsing column hits the floor and the wall, some cell's peak
    # pressure too (the waterfall's pool only deepens and the dam's block is still falling: their pressures peak at the end) - was set in a substep that is not
    # the last of its frame
    for c in (er.PRESSURE, er.SPEED):
        higher = env.planes[c] > r.per_frame.planes[c]
        print("   %s: %d cells peak between frames" % (er.NAMES[c], higher.sum()))
        assert not (env.planes[c] < r.per_frame.planes[c]).any()
        assert higher.any() or (c == er.PRESSURE and name in PRESSURE_PEAKS_AT_FRAME_ENDS)
    if name in ("dam", "wide"):      # tiles that never see water; in the wide flume the water also enters a tile that held none at frame 0
        entered = never = 0
        for ty in range(0, 136, 64):
            for tx in range(0, 264, 64):
                t = (slice(ty, ty + 64), slice(tx, tx + 64))
                entered += (not r.count0[t].any()) and bool(hit[t].any())
                never += not hit[t].any()
        print("   %d tiles entered, %d never wet" % (entered, never))
        assert never >= 6 and (entered >= 1 or name == "dam")
    if name == "wide":      # the box beside the left wall: the collapsing column's peak load falls between two frames, by a margin no solver mode's rounding closes
        x0, y0, x1, y1 = WALL_BOX
        b = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        peak, seen = float(env.f(er.PRESSURE)[b].max()), float(r.per_frame.f(er.PRESSURE)[b].max())
        print("   wall box: peak pressure %.6g, the largest a look per frame sees %.6g" % (peak, seen))
        assert peak > 1.01 * seen > 0


@pytest.mark.parametrize("name", ["waterfall", "dam"])
def test_edit_scene_buries_wet_cells(am, name):
    r = oracle_run(am, name, edit=True)
    x0, y0, x1, y1 = r.wall
    sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    assert r.wet_before.any() and r.solid[sl].all()      # the wall went up over water and still stands
    for c in er.CHANNELS:      # the buried cells keep the words they held when the wall went up
        assert (r.env.planes[c][sl] == r.at_edit.planes[c][sl]).all()
    assert (r.at_edit.planes[er.ARRIVAL][sl] != er.NEVER)[r.wet_before].all() and (r.at_edit.f(er.WET)[sl] > 0)[r.wet_before].all()
    free = oracle_run(am, name)      # ... while the run around them went another way than the one without the wall
    assert any((free.env.planes[c] != r.env.planes[c]).any() for c in er.CHANNELS)


def test_transports_and_forcing_change_the_planes(am):
    base = oracle_run(am, "flume")
    for kw in (dict(rk2=1), dict(rk2=1, mc=1), dict(forced=True), dict(heated=True)):
        other = oracle_run(am, "flume", **kw)
        assert (other.env.planes[er.ARRIVAL] != base.env.planes[er.ARRIVAL]).any(), kw
