"""The host half of the forcing (docs/forcing.md), no GPU: the numpy restatement (tests/forcing_ref.py) against its plain-loop twin on random grids,
euler_forcing_at against numpy doubles, the layout of both structs from a small C program, the host C code under the sanitizers
(tests/c/sanitize_forcing.c), and known answers on the CPU composition: free fall, the floor carries the weight at any gravity, no force no motion,
the sign of a sideways gravity, a pump drives a current."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import diagnostics_ref as dref
import euler_amd as ea
import forcing_ref as fref
import gauges_ref as gref
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ordered(x):
    """a float32 as an integer that grows with it: the distance of two such integers is the distance in ulps"""
    b = int(bits(x).reshape(-1)[0])
    return b if b < 0x80000000 else -(b - 0x80000000)


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("forcing_host"))


# ----------------------------------------------------------------------------- the two restatements
def random_scene(seed, X, Y, nboxes):
    rng = np.random.default_rng(seed)
    shape = (Y, X)
    solid = (rng.random(shape) < 0.2).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.6, rng.choice(np.array([1, 2, 8, 255], np.uint8), shape), 0).astype(np.uint8)
    utmp, vtmp = (rng.standard_normal(shape).astype(F32) * 3 for _ in range(2))
    for a in (utmp, vtmp):      # -0.f planted: x + 0.f is not x there
        hit = rng.random(shape) < 0.2
        a[hit] = rng.choice(np.array([-0.0, 0.0, 1e-30, -3.5], F32), int(hit.sum()))
    boxes = []
    for _ in range(nboxes):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya, yb = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
        boxes.append(((xa, ya, xb, yb), (float(F32(rng.standard_normal() * 20)), float(F32(rng.standard_normal() * 20)))))
    if nboxes >= 4:
        boxes[1] = boxes[0]                                        # a duplicate
        boxes[2] = ((1, 1, X - 2, Y - 2), (0.3, -0.0))             # the whole interior, over every other box
        boxes[3] = ((X - 2, Y - 2, X - 2, Y - 2), (1e4, -1e4))     # the last cell
    return solid, count, utmp, vtmp, boxes


@pytest.mark.parametrize("size,nboxes,acc", [((37, 23), 0, (0.0, -10.0)), ((37, 23), 7, (3.0, -8.0)), ((37, 23), 64, (-0.0, 0.0)), ((37, 23), 64, (1e-3, 7.0)),
                                              ((131, 70), 0, (2.5, 0.0)), ((131, 70), 33, (0.0, -10.0)), ((131, 70), 64, (-4.0, -9.81))])
def test_the_restatement_against_its_loop_twin(size, nboxes, acc):
    X, Y = size
    for seed in range(2):
        solid, count, utmp, vtmp, boxes = random_scene(1000 * nboxes + seed, X, Y, nboxes)
        dt = float(F32(0.0371))
        u1, v1, u2, v2 = utmp.copy(), vtmp.copy(), utmp.copy(), vtmp.copy()
        fref.apply_arrays(u1, v1, solid, count, acc, boxes, dt)
        fref.apply_loop(u2, v2, solid, count, acc, boxes, dt)
        assert np.array_equal(bits(u1), bits(u2)) and np.array_equal(bits(v1), bits(v2))
        lu, lv = fref.live_faces(solid, count)
        assert np.array_equal(bits(u1)[~lu], bits(utmp)[~lu]) and np.array_equal(bits(v1)[~lv], bits(vtmp)[~lv])      # a face that is not live is not touched
        if acc[0] == 0 and not nboxes:      # ax == 0 (-0.f too): u keeps its bits, planted -0.f included
            assert np.array_equal(bits(u1), bits(utmp)) and (bits(utmp)[lu] == 0x80000000).any()
        if acc[0] != 0:
            assert not (bits(u1)[lu] == 0x80000000).all()
        assert (bits(v1)[lv] != bits(vtmp)[lv]).any() or acc[1] == 0


def test_the_trap_an_unconditional_add_would_change_bits():
    z = np.array([-0.0], F32)
    assert bits(z + F32(0.0) * F32(0.1))[0] == 0 and bits(z)[0] == 0x80000000


# ----------------------------------------------------------------------------- euler_forcing_at
def test_forcing_at_against_numpy():
    rng = np.random.default_rng(7)
    worst = 0
    for k in range(400):
        g = rng.standard_normal(2) * 10
        shake = (rng.standard_normal() * 5, rng.standard_normal() * 5, abs(rng.standard_normal()) * 3, rng.standard_normal() * 4) if k % 4 else None
        f = fref.forcing(g, shake)
        rec = ea.forcing_record(g, shake)
        for t in (0.0, 0.1, float(rng.random() * 100), 12345.678):
            got, want = ea.forcing_at(rec, t), fref.forcing_at(f, t)
            for a, b in zip(got, want):
                ulp = abs(ordered(a) - ordered(b))
                worst = max(worst, ulp)
                assert ulp <= 1, (f, t, a, b)
                if shake is None:
                    assert bits(a) == bits(b) == bits(F32(g[0] if a is got[0] else g[1]))
    print("euler_forcing_at against numpy: at most %d float32 ulp" % worst)
    d = ea.forcing_default()
    assert ea.forcing_at(d, 3.25) == (F32(0), F32(-10)) and d.dtype == ea.FORCING_DTYPE and d["gy"] == -10 and d["nboxes"] == 0
    L = ea.load_library()
    out = np.zeros(2, F32)
    assert L.euler_forcing_at(None, 0.0, out.ctypes.data_as(L.euler_forcing_at.argtypes[2])) == -1 and L.euler_forcing_default(None) == -1


def test_dtypes_are_the_structs(tmp_path):
    f, b = ea.FORCING_DTYPE, ea.FORCE_BOX_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d", sizeof(euler_forcing), sizeof(euler_force_box), (int)EULER_FORCE_BOXES_MAX);\n'
                   + "".join('  printf(" %%zu", offsetof(euler_forcing, %s));\n' % n for n in f.names)
                   + "".join('  printf(" %%zu", offsetof(euler_force_box, %s));\n' % n for n in b.names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:3] == [48, 24, 64] == [f.itemsize, b.itemsize, ea.FORCE_BOXES_MAX]
    assert out[3:12] == [f.fields[n][1] for n in f.names] == [0, 4, 8, 12, 16, 24, 32, 36, 40]
    assert out[12:] == [b.fields[n][1] for n in b.names] == [0, 4, 8, 12, 16, 20]
    assert [f.fields[n][0] for n in f.names] == [np.float32] * 4 + [np.float64] * 2 + [np.int32] * 2 + [np.float64]
    assert [b.fields[n][0] for n in b.names] == [np.int32] * 4 + [np.float32] * 2


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the check of the record and the list, the tile-table builder, euler_forcing_at and the command's three spec parsers"""
    exe = str(tmp_path / "sanitize_forcing")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_forcing.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- known answers on the CPU composition
FALL_BOX = (27, 16, 36, 23)      # the 10 x 8 block of water of the free fall, air all around


def block_text(X, Y, box):
    """a scenario text with '0' over the cells of box (the first line fills row Y - 2, a line's first character column 1)"""
    x0, y0, x1, y1 = box
    rows = []
    for y in range(Y - 2, 0, -1):
        rows.append("".join("0" if (x0 <= x <= x1 and y0 <= y <= y1) else " " for x in range(1, X - 1)))
    return "\n".join(rows) + "\n"


def free_fall_check(u, v, solid, count, dt):
    """every live u face fl(3 dt), every live v face fl(-7 dt), every other face 0: exact"""
    lu, lv = fref.live_faces(solid, count)
    assert lu.sum() == 11 * 8 and lv.sum() == 10 * 9
    want_u = np.where(lu, F32(3) * F32(dt), F32(0)).astype(F32)
    want_v = np.where(lv, F32(-7) * F32(dt), F32(0)).astype(F32)
    assert np.array_equal(bits(u), bits(want_u)) and np.array_equal(bits(v), bits(want_v))


def test_free_fall(am):
    o = Oracle(64, 40).load_text(block_text(64, 40, FALL_BOX))
    assert int((o.count > 0).sum()) == 80
    dt = o.timestep(0.1)
    assert F32(dt) == F32(0.1)      # at rest: the frame time
    it = fref.substep(am, o, dt, fref.forcing((3, -7)), [], fref.Clock())
    assert it == 0 and not o.b.any()      # a uniform acceleration of a free block has no divergence: nothing to solve
    free_fall_check(np.array(o.u), np.array(o.v), np.array(o.solid), np.array(o.count), dt)
    o.close()


# The solve of this known answer runs to a tolerance of 1e-9 under a cap of 400 iterations, not the reference's 1e-6 under 100.  The bound below wants
# a == 0: the quantised pressures of the left and the right wall cancel to the last unit of 2^-8.  A wall cell k cells under the surface carries p = |gy| k,
# a value float32 holds exactly; (float)p is that value only when the solve's error stays under half a float32 ulp of it - 2.4e-7 at |gy| = 5 in the top
# row - and one ulp below it truncates to one unit less.  A residual of 1e-6 does not promise that (measured at 100 x 70, gy = -5: p off by up to 2e-6, one
# face one unit short, a = 2^-8); at 1e-9 the error is under 4e-9 at every size and gravity used here.  With gy = -10 the existing test meets the same bound
# at the default tolerance only because its smallest wall pressure, 10, has a float32 ulp twice as wide.
WEIGHT_TOL, WEIGHT_CAP = 1e-9, 400


def weight_bound(rec, gy):
    """|b - gy fluid| <= 1e-4 |gy| fluid and a == 0: test_gauges_host.py's hydrostatic bound, at gravity gy"""
    d = gref.derive(rec, gref.FORCE)
    fluid = int(rec["fluid"])
    print("gy %g fluid %d wetted faces %d: a = %.9g, b = %.9g, gy fluid = %.9g" % (gy, fluid, int(rec["terms"]), d["a"], d["b"], gy * fluid))
    assert fluid > 0 and abs(d["b"] - gy * fluid) <= 1e-4 * abs(gy) * fluid and d["a"] == 0
    return d


@pytest.mark.parametrize("size", [(64, 40), (100, 70)])
@pytest.mark.parametrize("gy", [-5.0, -20.0])
def test_weight_scales_with_gravity(am, size, gy):
    X, Y = size
    o = Oracle(X, Y).load_half_tank()
    o.c.tol, o.c.max_iterations = WEIGHT_TOL, WEIGHT_CAP
    it = fref.substep(am, o, o.timestep(0.1), fref.forcing((0, gy)), [], fref.Clock())
    assert it < WEIGHT_CAP      # under the cap: the solve converged
    rec = gref.gauge_ref(np.array(o.solid), np.array(o.count), np.array(o.u), np.array(o.v), np.array(o.p), gref.FORCE, (1, 1, X - 2, Y - 2))
    weight_bound(rec, gy)
    o.close()


def test_no_force_no_motion(am):
    o = Oracle(64, 40).load_half_tank()
    m0, c0 = o.markers.copy(), np.array(o.count)
    clock = fref.Clock()
    for _ in range(5):
        fref.step(am, o, fref.forcing((0, 0)), [], clock)
    assert not bits(o.u).any() and not bits(o.v).any()      # +0.f everywhere: bit for bit at rest
    assert np.array_equal(bits(o.markers), bits(m0)) and np.array_equal(o.count, c0)
    assert abs(clock.t - 0.5) < 1e-6
    o.close()


def com_x(o):
    return dref.derive(dref.diag_ref(np.array(o.solid), np.array(o.count), np.array(o.u), np.array(o.v)))["com_x"]


@pytest.mark.parametrize("gx", [2.0, -2.0])
def test_sideways_gravity_moves_the_centre_of_mass_its_way(am, gx):
    o = Oracle(64, 40).load_half_tank()
    x0 = com_x(o)
    clock = fref.Clock()
    for _ in range(10):
        fref.step(am, o, fref.forcing((gx, -10)), [], clock)
    x1 = com_x(o)
    print("gx %g: centre of mass x %.6f -> %.6f" % (gx, x0, x1))
    assert (x1 - x0) * gx > 0
    o.close()


PUMP = ((25, 6, 38, 12), (5.0, 0.0))      # fully under water in the 64 x 40 half tank (water: rows 2 .. 19)


def pump_flux(solid, count, u, v):
    (x0, y0, x1, y1), _ = PUMP
    xc = (x0 + x1) // 2
    rec = gref.gauge_ref(solid, count, u, v, None, gref.FLUX, (xc, y0, xc, y1))
    assert int(rec["fluid"]) == y1 - y0 + 1      # under water
    return gref.derive(rec, gref.FLUX)["a"]


def test_a_pump_drives_a_current(am):
    o = Oracle(64, 40).load_half_tank()
    clock = fref.Clock()
    for _ in range(5):
        fref.step(am, o, fref.forcing(), [PUMP], clock)
    a = pump_flux(np.array(o.solid), np.array(o.count), np.array(o.u), np.array(o.v))
    print("flux through the pump's centre column after 5 frames: %.6f" % a)
    assert a > 0
    o.close()
