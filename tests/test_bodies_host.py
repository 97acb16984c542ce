"""The host half of the moving bodies (docs/bodies.md), no GPU: the numpy restatement (tests/bodies_ref.py) against its plain-loop twin on random scenes,
euler_body_at against numpy doubles, the layout of both structs from a small C program, the host C code under the sanitizers (tests/c/sanitize_bodies.c),
and known answers on the CPU composition: a piston in a lidded channel drives wx times its wet face through every section, a shift keeps every marker, a body
at rest is the wall of the same SOLID edit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import bodies_ref as bref
import euler_amd as ea
import forcing_ref as fref
from euler_amd import scenarios
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("bodies_host"))


def record(b):
    return ea.body((b["w"], b["h"]), (b["x"], b["y"]), (b["vx"], b["vy"]), (b["amp_x"], b["amp_y"]), b["hz"], b["phase"])


def lib_at(b, t, X, Y):
    """euler_body_at in the shape of bodies_ref.body_at"""
    st = ea.body_at(record(b), t, X, Y)
    return float(st["px"]), float(st["py"]), int(st["ox"]), int(st["oy"])


# ----------------------------------------------------------------------------- the two restatements
def random_scene(seed, X, Y, nbodies):
    """masks, counts and markers at random (markers also in solid cells, on cell edges and one ulp below them), bodies anywhere inside the clamp range -
    overlapping ones included - with targets up to two cells away on either axis"""
    rng = np.random.default_rng(seed)
    shape = (Y, X)
    r = rng.random(shape)
    solid, sink, source = ((lo <= r) & (r < hi) for lo, hi in ((0.0, 0.15), (0.15, 0.2), (0.2, 0.25)))
    n = 6 * X * Y // 5
    m = np.stack([rng.uniform(1, X - 1, n), rng.uniform(1, Y - 1, n)], axis=1).astype(F32)
    edge = rng.random(n) < 0.1
    m[edge, 0] = np.floor(m[edge, 0])
    below = edge & (rng.random(n) < 0.5)
    m[below, 0] = np.nextafter(m[below, 0], F32(-np.inf))
    edge = rng.random(n) < 0.1
    m[edge, 1] = np.floor(m[edge, 1])
    count = (np.bincount(np.floor(m[:, 1]).astype(int) * X + np.floor(m[:, 0]).astype(int), minlength=X * Y).reshape(shape) % 256).astype(np.uint8)
    bodies, origins, tgt = [], [], []
    for _ in range(nbodies):
        w, h = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        ox, oy = int(rng.integers(2, X - 2 - w + 1)), int(rng.integers(2, Y - 2 - h + 1))
        tx = int(np.clip(ox + rng.integers(-2, 3), 2, X - 2 - w))
        ty = int(np.clip(oy + rng.integers(-2, 3), 2, Y - 2 - h))
        bodies.append(bref.body((w, h), (ox, oy)))
        origins.append([ox, oy])
        tgt.append((tx, ty, F32(0), F32(0)))
    return m, solid.astype(np.uint8), source.astype(np.uint8), sink.astype(np.uint8), count, bodies, origins, tgt


@pytest.mark.parametrize("size,nbodies", [((37, 23), 1), ((37, 23), 5), ((37, 23), 16), ((131, 70), 3), ((131, 70), 16)])
def test_the_restatement_against_its_loop_twin(size, nbodies):
    X, Y = size
    moved = pushed = 0
    for seed in range(2):
        m, solid, source, sink, count, bodies, origins, tgt = random_scene(100 * nbodies + seed, X, Y, nbodies)
        a = [x.copy() for x in (m, solid, source, sink, count)]
        b = [x.copy() for x in (m, solid, source, sink, count)]
        oa, ob = [list(o) for o in origins], [list(o) for o in origins]
        na = bref.begin_arrays(*a, bodies, oa, tgt)
        nb = bref.begin_loops(*b, bodies, ob, tgt)
        assert na == nb == sum(abs(t[0] - o[0]) + abs(t[1] - o[1]) for t, o in zip(tgt, origins))
        assert oa == ob == [[t[0], t[1]] for t in tgt]
        assert np.array_equal(bits(a[0]), bits(b[0]))
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y)
        assert len(a[0]) == len(m)      # a shift deletes nothing and keeps the array's order
        moved += na
        pushed += int((bits(a[0]) != bits(m)).any(axis=1).sum())
        if na:      # behind the shifts every rectangle is solid, whatever another body's CLEAR did
            for bd, o in zip(bodies, oa):
                sl = bref._sl(bref.rect(bd, o))
                assert a[1][sl].all() and not a[2][sl].any() and not a[3][sl].any() and not a[4][sl].any()
        else:
            assert np.array_equal(a[1], solid)
    assert moved > 0 and pushed > 0


def test_plan_is_x_first():
    assert bref.plan(5, 5, 5, 5) == []
    assert bref.plan(5, 5, 7, 4) == [(0, 1), (0, 1), (1, -1)]
    assert bref.plan(5, 5, 4, 7) == [(0, -1), (1, 1), (1, 1)]
    assert bref.strips(10, 20, 3, 5, 0, 1) == ((13, 20, 13, 24), (10, 20, 10, 24))
    assert bref.strips(10, 20, 3, 5, 1, -1) == ((10, 19, 12, 19), (10, 24, 12, 24))


# ----------------------------------------------------------------------------- euler_body_at
def test_body_at_against_numpy():
    rng = np.random.default_rng(11)
    X, Y = 131, 70
    worst, ties = 0.0, 0
    for k in range(400):
        w, h = int(rng.integers(1, X - 3)), int(rng.integers(1, Y - 3))
        b = bref.body((w, h), (rng.uniform(-20, X + 20), rng.uniform(-20, Y + 20)), rng.uniform(-10, 10, 2),
                      rng.uniform(-8, 8, 2) if k % 3 else (0.0, 0.0), abs(rng.standard_normal()) if k % 3 else 0.0, rng.standard_normal() * 3)
        for t in (0.0, 0.1, float(rng.random() * 50), 1234.5):
            got, want = lib_at(b, t, X, Y), bref.body_at(b, t, X, Y)
            worst = max(worst, abs(got[0] - want[0]), abs(got[1] - want[1]))
            assert abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9, (b, t, got, want)
            assert 2 <= got[2] <= X - 2 - w and 2 <= got[3] <= Y - 2 - h
            assert got[2] == int(np.floor(got[0] + 0.5)) and got[3] == int(np.floor(got[1] + 0.5))
            if b["hz"] == 0.0:      # no sin: the same doubles
                assert got == want
    print("euler_body_at against numpy: at most %.3g cells apart" % worst)
    # ties and clamps, exactly
    b = bref.body((3, 2), (10.5, 20.5))
    assert lib_at(b, 0.0, X, Y) == (10.5, 20.5, 11, 21)
    b = bref.body((3, 2), (float(np.nextafter(10.5, 0)), 2.0), (-1.0, 4.0))
    assert lib_at(b, 0.0, X, Y)[2:] == (10, 2) and lib_at(b, 100.0, X, Y) == (2.0, float(Y - 4), 2, Y - 4)
    L = ea.load_library()
    st = np.zeros((), ea.BODY_STATE_DTYPE)
    assert L.euler_body_at(None, 0.0, X, Y, st.ctypes.data) == -1 and L.euler_body_at(record(b).ctypes.data, 0.0, X, Y, None) == -1
    big = record(bref.body((X - 3, 1), (2, 2)))
    assert L.euler_body_at(big.ctypes.data, 0.0, X, Y, st.ctypes.data) == -1


def test_dtypes_are_the_structs(tmp_path):
    b, s = ea.BODY_DTYPE, ea.BODY_STATE_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d", sizeof(euler_body), sizeof(euler_body_state), (int)EULER_BODIES_MAX);\n'
                   + "".join('  printf(" %%zu", offsetof(euler_body, %s));\n' % n for n in b.names)
                   + "".join('  printf(" %%zu", offsetof(euler_body_state, %s));\n' % n for n in s.names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:3] == [64, 24, 16] == [b.itemsize, s.itemsize, ea.BODIES_MAX]
    assert out[3:14] == [b.fields[n][1] for n in b.names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56]
    assert out[14:] == [s.fields[n][1] for n in s.names] == [0, 8, 16, 20]
    assert [b.fields[n][0].base for n in b.names] == [np.float64] * 4 + [np.float32] * 4 + [np.int32] * 3 and b.fields["reserved"][0].shape == (2,)
    assert [s.fields[n][0] for n in s.names] == [np.float64] * 2 + [np.int32] * 2


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the check of the list, euler_body_at, the shift plans and strips, the perimeter enumeration and the command's spec parser"""
    probe = tmp_path / "probe.c"      # are the sanitizers' runtimes installed at all?  Asked before any work, so that no failure of the real build is taken for it
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run(["gcc", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("libasan / libubsan not installed")
    exe = str(tmp_path / "sanitize_bodies")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_bodies.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- known answers on the CPU composition
# A lidded channel full of water: floor in row 2, lid in row CH_Y1 + 1, water in rows CH_Y0 .. CH_Y1 from the left wall to column CH_X1, air beyond it up to
# the right wall.  The piston is PISTON_W cells thick, as high as the channel, and starts PISTON_X cells in.
PISTON_GRID = (48, 14)
CH_Y0, CH_Y1, CH_X1 = 3, 8, 34
PISTON_W, PISTON_X = 2, 6
PISTON_CAP = 2000      # iterations allowed: the solve must stop on its tolerance, not here


def channel_text(X, Y):
    """the first line fills row Y - 2, a line's first character column 1"""
    rows = []
    for y in range(Y - 2, 0, -1):
        if y == CH_Y0 - 1 or y == CH_Y1 + 1:
            rows.append("X" * (CH_X1 + 6))      # floor and lid reach a little beyond the water
        elif CH_Y0 <= y <= CH_Y1:
            rows.append("0" * CH_X1)
        else:
            rows.append("")
    return "\n".join(rows) + "\n"


def piston(vx):
    return bref.body((PISTON_W, CH_Y1 - CH_Y0 + 1), (PISTON_X, CH_Y0), (vx, 0.0))


def piston_sections(u, v, p, solid, count, origin, wx, dt, tol, iters):
    """The known answer and its margin.  With h = 1 and density 1 the system is A p = b, b_i = -div_i / dt (eo_build_system: the divergence of utmp / vtmp over
    the four faces of a fluid cell, the piston's face holding wx), and the update is u = utmp - dt grad p on fluid faces.  In exact arithmetic the divergence the
    update leaves in cell i - taking the wall's wx on the piston's face - is therefore -dt r_i, r = b - A p.  The solve stops at max |r_i| <= tol.  Summing the
    cells of the columns between the piston's face and a section, inner faces cancel, the lid's and the floor's faces are solid (v = 0), and what is left is
    flux(section) - wx rows.  So |flux - wx rows| <= cells dt tol, plus:
      - the solver's r is updated by recurrence, 2 roundings of at most 2^-53 |alpha (A s)_i| per iteration; |alpha A s| <= 8 max |p| bounds each: iters 2^-52 8 max|p| per cell, times dt;
      - each face of the section is fl(utmp + fl(fl(-(float)dp) dt)): three roundings of 2^-24 relative, at most 2^-24 (2 |g| + |u|) (1 + 2^-20) with g = dt dp;
      - the sum of `rows` floats in double: exact to 2^-52 relative, taken as rows 2^-52 |u| max."""
    ox, oy = origin
    rows = range(CH_Y0, CH_Y1 + 1)
    wet_rows = sum(1 for y in rows if count[y, ox + PISTON_W] and not solid[y, ox + PISTON_W])
    assert wet_rows == len(rows)
    want = float(wx) * wet_rows
    pmax = float(np.abs(p).max())
    worst = 0.0
    first, last = ox + PISTON_W, CH_X1      # the water columns in front of the piston; section x is the right faces of column x
    assert count[CH_Y0:CH_Y1 + 1, first:last + 1].all() and not count[CH_Y0:CH_Y1 + 1, last + 1].any()
    for x in range(first, last + 1):
        faces = np.array([u[y, x] for y in rows], np.float64)
        g = np.array([dt * (p[y, x + 1] - p[y, x]) for y in rows], np.float64)
        cells = (x - first + 1) * len(rows)
        margin = cells * dt * (tol + iters * 2.0 ** -52 * 8 * pmax)
        margin += float(np.sum(2.0 ** -24 * (2 * np.abs(g) + np.abs(faces)) * (1 + 2.0 ** -20)))
        margin += len(rows) * 2.0 ** -52 * float(np.abs(faces).max())
        err = abs(float(faces.sum()) - want)
        print("section %2d: flux %.9g, wanted %.9g, off by %.3g, margin %.3g" % (x, faces.sum(), want, err, margin))
        assert err <= margin, (x, err, margin)
        worst = max(worst, err / margin)
    # and the piston's own faces hold 0 behind the update, the lid's and the floor's too
    assert not u[CH_Y0:CH_Y1 + 1, ox + PISTON_W - 1].any() and not u[CH_Y0:CH_Y1 + 1, ox - 1].any()
    assert not v[CH_Y1, first:last + 1].any() and not v[CH_Y0 - 1, first:last + 1].any()
    return worst


@pytest.mark.parametrize("vx", [4.0, 0.75])
def test_a_piston_drives_wx_times_its_face_through_every_section(vx):
    X, Y = PISTON_GRID
    o = Oracle(X, Y).load_text(channel_text(X, Y))
    o.c.tile_records = 0
    o.c.max_iterations = PISTON_CAP
    bodies = [piston(vx)]
    origins = bref.set_bodies(o, [], [], bodies, 0.0, at=lib_at)      # (the positions are euler_body_at's own: no libm between the test and the library)
    assert origins == [[PISTON_X, CH_Y0]]
    dt = float(F32(0.05))
    tgt = bref.targets(bodies, 0.0, dt, X, Y, at=lib_at)
    assert tgt[0][2] == F32(vx) and tgt[0][3] == 0      # the mean velocity of a uniform motion is the velocity
    o.utmp[...] = 0
    o.vtmp[...] = 0
    it = bref.project_stage(o, dt, bodies, origins, tgt)
    assert 0 < it < PISTON_CAP and o.c.last_residual <= o.c.tol      # converged
    assert (np.array(o.p) >= 0).all() and np.array(o.p).max() > 0      # the piston compresses: the clamp p >= 0 took nothing away
    piston_sections(np.array(o.u), np.array(o.v), np.array(o.p), np.array(o.solid), np.array(o.count), origins[0], tgt[0][2], dt, float(o.c.tol), it)
    assert not o.utmp.any() and not o.vtmp.any()      # the wall velocity is withdrawn behind the stage
    o.close()


def test_a_shift_keeps_every_marker_where_the_landing_cells_are_free(am):
    """the piston run for a while: it shifts, the water in front is pushed and none is lost (the channel is open at its far end: nothing lands in a wall)"""
    X, Y = PISTON_GRID
    o = Oracle(X, Y).load_text(channel_text(X, Y))
    o.c.tile_records = 0
    o.c.max_iterations = PISTON_CAP
    bodies = [piston(4.0)]
    origins = bref.set_bodies(o, [], [], bodies, 0.0, at=lib_at)
    n0 = o.n_markers
    ahead0 = int((np.floor(o.markers[:, 0]) >= PISTON_X + PISTON_W).sum())
    clock = fref.Clock()
    f = fref.forcing((0.0, 0.0))      # no gravity: the water stays in the channel's rows
    shifts = 0
    for _ in range(10):
        before = [list(og) for og in origins]
        bref.step(am, o, bodies, origins, clock, f, at=lib_at)
        shifts += abs(origins[0][0] - before[0][0])
        assert o.n_markers == n0
        sl = bref._sl(bref.rect(bodies[0], origins[0]))
        assert o.solid[sl].all() and not o.count[sl].any()
    assert shifts >= 3 and origins[0] == [lib_at(bodies[0], clock.t, X, Y)[2], CH_Y0]
    assert int((np.floor(o.markers[:, 0]) >= origins[0][0] + PISTON_W).sum()) == ahead0 > 0      # the water in front of the piston is still in front of it
    o.close()


def test_a_body_at_rest_is_the_wall_of_the_same_edit(am):
    X, Y = 96, 64
    text = scenarios.dam_break()
    box = (12, 2, 14, 9)      # in the falling block's way
    a, b = Oracle(X, Y).load_text(text, upscale=True), Oracle(X, Y).load_text(text, upscale=True)
    # a: the composition with a body that never moves (an amplitude with hz = 0 and a phase: sin is constant)
    body = bref.body((3, 8), (12.0, 2.0), (0.0, 0.0), (0.25, 0.0), 0.0, 1.0)
    origins = bref.set_bodies(a, [], [], [body], 0.0, at=lib_at)
    assert origins == [[12, 2]]
    # b: the oracle's own run behind the same SOLID edit
    sl = bref._sl(box)
    b.set_markers(bref.delete_in_box(b.markers, box))
    b.solid[sl], b.source[sl], b.sink[sl], b.count[sl] = 1, 0, 0, 0
    clock = fref.Clock()
    for k in range(30):
        bref.step(am, a, [body], origins, clock, at=lib_at)
        b.step()
        for n in ("u", "v", "utmp", "vtmp", "count", "prev_count", "solid", "source", "sink"):
            assert np.array_equal(np.array(getattr(a, n)).view(np.uint8), np.array(getattr(b, n)).view(np.uint8)), (k, n)
        assert np.array_equal(bits(a.markers), bits(b.markers)) and a.c.rng_state == b.c.rng_state
    assert np.abs(a.u).max() > 0.5 and origins == [[12, 2]]
    a.close(); b.close()
