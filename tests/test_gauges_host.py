"""The host half of the batched gauges (docs/gauges.md), no GPU: the numpy restatement (tests/gauges_ref.py) against its plain-loop twin on random
grids and on hand-worked cases, euler_gauge_derive against Python doubles, the layout of both structs from a small C program, the host C code under the
sanitizers (tests/c/sanitize_gauges.c), and a known answer: the floor of a tank at rest carries the weight of the water (CPU oracle)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import gauges_ref as gref
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (ea.GAUGE_LEVEL, ea.GAUGE_PRESSURE, ea.GAUGE_FORCE, ea.GAUGE_FLUX)      # (the header's; gauges_ref has its own)
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5000.0, -4096.5, 1e30, -3e38, 4095.99], np.float32)


def random_grids(seed, X=37, Y=23):
    rng = np.random.default_rng(seed)
    shape = (Y, X)
    solid = (rng.random(shape) < 0.2).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.7, rng.choice(np.array([1, 2, 8, 255], np.uint8), shape), 0).astype(np.uint8)
    u, v = (rng.standard_normal(shape).astype(np.float32) * 3 for _ in range(2))
    p = np.abs(rng.standard_normal(shape)) * 50.0
    for a, special in ((u, SPECIAL), (v, SPECIAL), (p, np.array([np.nan, np.inf, -np.inf, -5.0, 1e30, 16777217.0, 3e-3, 0.0]))):
        hit = rng.random(shape) < 0.05
        a[hit] = rng.choice(special, int(hit.sum()))
    return solid, count, u, v, p


def random_boxes(rng, X, Y, n):
    out = []
    for _ in range(n):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya, yb = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
        out.append((xa, ya, xb, yb))
    return out


def test_dtypes_are_the_structs(tmp_path):
    d, g = ea.GAUGE_REC_DTYPE, ea.GAUGE_DTYPE
    assert d.itemsize == 72 and d == gref.DTYPE and g.itemsize == 24 and g == gref.GAUGE_DTYPE
    assert (ea.GAUGE_LEVEL, ea.GAUGE_PRESSURE, ea.GAUGE_FORCE, ea.GAUGE_FLUX, ea.GAUGES_MAX) == (0, 1, 2, 3, 1024) == KINDS + (1024,)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d %d %d", sizeof(euler_gauge), sizeof(euler_gauge_rec), sizeof(euler_gauge_values), (int)EULER_GAUGE_LEVEL, (int)EULER_GAUGE_PRESSURE,'
                   ' (int)EULER_GAUGE_FORCE, (int)EULER_GAUGE_FLUX, (int)EULER_GAUGES_MAX);\n'
                   + "".join('  printf(" %%zu", offsetof(euler_gauge, %s));\n' % f for f in g.names)
                   + "".join('  printf(" %%zu", offsetof(euler_gauge_rec, %s));\n' % f for f in d.names)
                   + "".join('  printf(" %%zu", offsetof(euler_gauge_values, %s));\n' % f for f in ea.GAUGE_VALUES) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:8] == [24, 72, 8 * len(ea.GAUGE_VALUES), 0, 1, 2, 3, 1024]
    assert out[8:14] == [g.fields[f][1] for f in g.names] == [0, 4, 8, 12, 16, 20]
    assert out[14:28] == [d.fields[f][1] for f in d.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 68]
    assert out[28:] == [0, 8, 16, 24]
    assert [d.fields[f][0] for f in d.names] == [np.uint32] * 8 + [np.uint64] * 4 + [np.float32] * 2
    assert [g.fields[f][0] for f in g.names] == [np.int32] * 6


@pytest.mark.parametrize("seed", range(4))
def test_the_restatement_against_its_loop_twin_on_random_grids(seed):
    grids = random_grids(seed)
    rng = np.random.default_rng(100 + seed)
    boxes = [(1, 1, 35, 21), (1, 1, 1, 1), (35, 21, 35, 21), (1, 7, 35, 7), (9, 1, 9, 21)] + random_boxes(rng, 37, 23, 6)
    seen = {n: 0 for n in gref.DTYPE.names}
    for box in boxes:
        for kind in KINDS:
            a, b = gref.gauge_ref(*grids, kind, box), gref.gauge_loop(*grids, kind, box)
            assert not gref.mismatches(a, b), (box, kind, a, b)
            for n in seen:
                seen[n] += int(a[n] != 0)
    assert all(seen.values()), seen      # every field was exercised
    whole = gref.gauge_ref(*grids, gref.FLUX, boxes[0])
    assert whole["nonfinite"] > 0 and np.isinf(whole["max_a"]) and min(int(whole[n]) for n in ("a_pos", "a_neg", "b_pos", "b_neg")) >= 4096 << 20      # saturated terms among them
    whole = gref.gauge_ref(*grids, gref.PRESSURE, boxes[0])
    assert whole["nonfinite"] > 0 and np.isinf(whole["max_a"]) and whole["a_pos"] >= 1 << 32
    whole = gref.gauge_ref(*grids, gref.FORCE, boxes[0])
    assert whole["terms"] > whole["fluid"] // 4 and min(int(whole[n]) for n in ("a_pos", "a_neg", "b_pos", "b_neg")) > 0


def _blank(X=9, Y=7):
    return [np.zeros((Y, X), np.uint8), np.zeros((Y, X), np.uint8), np.zeros((Y, X), np.float32), np.zeros((Y, X), np.float32), np.zeros((Y, X), np.float64)]


def _both(grids, kind, box):
    a, b = gref.gauge_ref(*grids, kind, box), gref.gauge_loop(*grids, kind, box)
    assert not gref.mismatches(a, b), (a, b)
    return a


def _fields(r, **want):
    for n, val in want.items():
        assert (np.float32(r[n]).view(np.uint32) == np.float32(val).view(np.uint32)) if n in gref.FLOATS else (int(r[n]) == val), (n, r[n], val)


def test_one_fluid_cell_walled_on_three_sides():
    solid, count, u, v, p = g = _blank()
    count[3, 4] = 2
    solid[3, 3] = solid[3, 5] = solid[2, 4] = 1      # left, right, below; open above
    p[3, 4] = 12.5
    box = (3, 2, 5, 4)
    _fields(_both(g, gref.LEVEL, box), cells=9, fluid=1, lo_x=4, hi_x=4, lo_y=3, hi_y=3, terms=0, nonfinite=0, a_pos=0, a_neg=0, b_pos=0, b_neg=0, max_a=0.0, max_b=0.0)
    _fields(_both(g, gref.PRESSURE, box), cells=9, fluid=1, terms=1, a_pos=3200, a_neg=0, max_a=12.5, max_b=0.0)
    _fields(_both(g, gref.FORCE, box), fluid=1, terms=3, a_pos=3200, a_neg=3200, b_pos=0, b_neg=3200, max_a=12.5, max_b=12.5, nonfinite=0)
    # the force is defined from the fluid side: a box of the one cell sees the walls outside it, a box of a wall alone sees nothing
    _fields(_both(g, gref.FORCE, (4, 3, 4, 3)), cells=1, fluid=1, terms=3, a_pos=3200, a_neg=3200, b_neg=3200)
    _fields(_both(g, gref.FORCE, (5, 3, 5, 3)), cells=1, fluid=0, lo_x=gref.NONE, hi_x=0, lo_y=gref.NONE, hi_y=0, terms=0, a_pos=0, a_neg=0)
    # the faces: both sides walled (dead), the top face open and live, the face below dead; the face above the LEFT wall is dead, the one above the cell itself carries v
    u[3, 4], u[3, 3], v[3, 4], v[2, 4] = 1.5, 2.5, -0.75, 4.0
    _fields(_both(g, gref.FLUX, box), terms=1, a_pos=0, a_neg=0, b_pos=0, b_neg=int(0.75 * 2**20), max_a=0.0, max_b=0.75)
    solid[3, 5] = 0      # the right wall opens: its face is live and carries u
    _fields(_both(g, gref.FLUX, box), terms=2, a_pos=int(1.5 * 2**20), b_neg=int(0.75 * 2**20), max_a=1.5)
    _fields(_both(g, gref.FORCE, box), terms=2, a_pos=0, a_neg=3200, b_neg=3200)
    # a dry cell beside water: its right face is live through the neighbour's count
    _fields(_both(g, gref.FLUX, (5, 3, 5, 3)), fluid=0, terms=0)
    count[3, 6], u[3, 5] = 3, -2.0
    _fields(_both(g, gref.FLUX, (5, 3, 5, 3)), fluid=0, lo_x=gref.NONE, hi_x=0, terms=1, a_pos=0, a_neg=2 << 20, max_a=2.0, b_pos=0, b_neg=0)


def test_planted_pressures_and_velocities():
    solid, count, u, v, p = g = _blank(12, 6)
    count[2, 1:11] = 1
    solid[1, :] = 1      # a floor under the row of water
    vals = [np.nan, np.inf, -np.inf, -5.0, 1e30, 16777217.0, 3e-3, 0.5, 2.0**-8, 7.0]
    p[2, 1:11] = vals
    r = _both(g, gref.PRESSURE, (1, 2, 10, 2))
    # NaN: counted, nothing added; +inf and the huge ones saturate at 2^24 * 2^8; -inf, -5 and 3e-3 add 0; 0.5 -> 128; 2^-8 -> 1; 7 -> 1792
    _fields(r, fluid=10, terms=10, nonfinite=1, a_pos=3 * (1 << 32) + 128 + 1 + 1792, a_neg=0, max_a=np.inf)
    r = _both(g, gref.FORCE, (1, 2, 10, 2))
    _fields(r, fluid=10, terms=10, nonfinite=1, b_neg=3 * (1 << 32) + 128 + 1 + 1792, b_pos=0, a_pos=0, a_neg=0, max_b=np.inf, max_a=0.0)
    r = _both(g, gref.PRESSURE, (4, 2, 4, 2))
    _fields(r, fluid=1, a_pos=0, max_a=0.0, nonfinite=0)      # a negative pressure: clamped to 0
    r = _both(g, gref.PRESSURE, (8, 2, 10, 2))
    _fields(r, a_pos=128 + 1 + 1792, max_a=7.0)
    # velocities: above 4096 saturates, -0.f is positive, NaN is counted once per cell even when both faces are NaN
    u[2, 1:8] = [5000.0, -4096.5, -0.0, np.nan, np.inf, -np.inf, 4095.99]
    v[2, 4] = np.nan
    r = _both(g, gref.FLUX, (1, 2, 7, 2))
    q = int(np.float32(4095.99) * np.float32(2**20))
    _fields(r, fluid=7, terms=14, nonfinite=1, a_pos=(4096 << 20) * 2 + q, a_neg=(4096 << 20) * 2, b_pos=0, b_neg=0, max_a=np.inf, max_b=0.0)
    r = _both(g, gref.FLUX, (3, 2, 3, 2))      # -0.f alone: on the positive side, with 0
    _fields(r, terms=2, a_pos=0, a_neg=0, nonfinite=0, max_a=0.0)
    r = _both(g, gref.FLUX, (1, 2, 2, 2))
    _fields(r, a_pos=4096 << 20, a_neg=4096 << 20, max_a=5000.0)


def test_derive_against_python_doubles():
    rng = np.random.default_rng(5)
    recs = np.zeros(40, ea.GAUGE_REC_DTYPE)
    recs["fluid"] = rng.integers(0, 3, 40) * rng.integers(1, 1 << 20, 40)
    recs["terms"] = rng.integers(0, 3, 40) * rng.integers(1, 1 << 20, 40)
    recs["lo_y"], recs["hi_y"] = rng.integers(1, 50, 40), rng.integers(50, 9000, 40)
    for n in ("a_pos", "a_neg", "b_pos", "b_neg"):
        recs[n] = rng.integers(0, 1 << 62, 40, dtype=np.uint64) >> rng.integers(0, 60, 40).astype(np.uint64)
    recs["a_pos"][0], recs["a_neg"][0], recs["fluid"][0], recs["terms"][0] = (1 << 60) + 4096, (1 << 60) - 512, 7, 3      # sums near 2^60
    recs["b_pos"][1], recs["b_neg"][1], recs["fluid"][1] = (1 << 60) - 1, (1 << 60) + 1, 1      # ... not exact in a double: the same rounding on both sides
    assert (recs["fluid"] == 0).any() and ((recs["terms"] == 0) & (recs["fluid"] > 0)).any()
    for r in recs:
        for kind in KINDS:
            got, want = ea.gauge_derive(r, kind), gref.derive(r, kind)
            assert set(got) == set(ea.GAUGE_VALUES) == set(want)
            for k in want:
                assert got[k] == want[k], (kind, k, got[k], want[k])
    assert gref.derive(recs[0], gref.PRESSURE)["a"] == 4608 / 256 and gref.derive(recs[0], gref.FLUX)["a"] == 4608 / 2**20
    empty = np.zeros((), ea.GAUGE_REC_DTYPE)
    empty["a_pos"], empty["lo_y"], empty["lo_x"] = 999, gref.NONE, gref.NONE
    assert all(val == 0.0 for val in ea.gauge_derive(empty, ea.GAUGE_FORCE).values())
    L = ea.load_library()
    out = np.zeros(4)
    assert L.euler_gauge_derive(None, 0, out.ctypes.data) == -1 and L.euler_gauge_derive(empty.ctypes.data, 0, None) == -1
    assert L.euler_gauge_derive(empty.ctypes.data, 4, out.ctypes.data) == -1 and L.euler_gauge_derive(empty.ctypes.data, -1, out.ctypes.data) == -1
    with pytest.raises(ea.EulerError):
        ea.gauge_derive(empty, 9)


def test_the_csv_line():
    r = np.zeros((), gref.DTYPE)
    r["cells"], r["fluid"], r["lo_x"], r["hi_x"], r["lo_y"], r["hi_y"], r["terms"] = 12, 5, 3, 4, 1, 9, 5
    r["a_pos"], r["a_neg"], r["b_neg"], r["max_a"], r["max_b"], r["nonfinite"] = 3200, 640, 1, 12.5, 0.1, 2
    assert gref.csv_line(7, 3, gref.FORCE, r) == "7,3,force,12,5,3,4,1,9,5,10,-0.00390625,12.5,0.100000001,2\n"
    assert gref.csv_line(0, 0, gref.FLUX, r) == "0,0,flux,12,5,3,4,1,9,5,0.00244140625,-9.53674316e-07,12.5,0.100000001,2\n"
    r["fluid"] = 0
    r["lo_x"] = r["lo_y"] = gref.NONE
    assert gref.csv_line(1, 2, gref.LEVEL, r) == "1,2,level,12,0,4294967295,4,4294967295,9,5,0,0,12.5,0.100000001,2\n"
    assert gref.CSV_HEADER.count(",") == gref.csv_line(1, 2, gref.LEVEL, r).count(",") == 14


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the list check, the chunk-table builder, euler_gauge_derive and the command's spec parser and line formatter"""
    exe = str(tmp_path / "sanitize_gauges")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_gauges.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- a known answer: the floor carries the weight
def hydrostatic_bound(rec):
    """A column at rest has p = 10 k at its k-th fluid cell from the top (main.c:705-706, 787-800, gravity -10): the floor carries the weight of the water,
    b = -10 fluid, and the side walls cancel, a = 0.  The margin: at most 2^-8 of quantisation per wetted face against face pressures of at least 10, and a
    solver tolerance of 1e-6."""
    d = gref.derive(rec, gref.FORCE)
    weight = 10.0 * int(rec["fluid"])
    print("fluid %d wetted faces %d: a = %.9g, b = %.9g, weight %.9g" % (int(rec["fluid"]), int(rec["terms"]), d["a"], d["b"], weight))
    assert int(rec["fluid"]) > 0 and abs(d["b"] + weight) <= 1e-4 * weight and d["a"] == 0
    return d


@pytest.mark.parametrize("size", [(64, 40), (100, 70), (130, 70)])
def test_hydrostatic_floor_force_on_the_oracle(size):
    Xg, Yg = size
    o = Oracle(Xg, Yg).load_half_tank()
    o.substep(o.timestep(0.1))
    assert o.c.last_pcg_iterations < 100      # under the cap: the solve converged
    g = [np.array(a) for a in (o.solid, o.count, o.u, o.v, o.p)]
    whole = (1, 1, Xg - 2, Yg - 2)
    rec = gref.gauge_ref(*g, gref.FORCE, whole)
    assert not gref.mismatches(rec, gref.gauge_loop(*g, gref.FORCE, whole))
    hydrostatic_bound(rec)
    assert rec["nonfinite"] == 0 and rec["b_pos"] == 0 and rec["a_pos"] == rec["a_neg"] > 0
    # the same through the product's derive
    assert ea.gauge_derive(rec.astype(ea.GAUGE_REC_DTYPE), ea.GAUGE_FORCE) == gref.derive(rec, gref.FORCE)
    o.close()
