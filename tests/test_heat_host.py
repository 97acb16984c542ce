"""The host half of the temperature (docs/heat.md), no GPU: the numpy restatement (tests/heat_ref.py) against its plain-loop twin on random scenes, the
layout of both structs from a small C program, the host C code under the sanitizers (tests/c/sanitize_heat.c), and known answers on the CPU composition:
a passive scalar and a uniform field leave the oracle's run untouched, diffusion conserves heat, the maximum principle, a hot blob rises and a cold one
sinks (and the other way round when gravity points up), a heater on the floor drives an upward flux; the raster's restatement on planted NaN and
infinities, and euler_heat_paint against numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import advect_maccormack_ref as amref
import euler_amd as ea
import forcing_ref as fref
import gauges_ref as gref
import heat_ref as href
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U24 = 2.0 ** -24      # the relative rounding error of one float32 operation


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return amref.build(tmp_path_factory.mktemp("heat_host"))


# ----------------------------------------------------------------------------- the two restatements
def random_scene(seed, X, Y, nboxes, ambient):
    """solid, count (the border ring dry, as in every scene: it is all sink), T with the dry cells at ambient, utmp / vtmp with -0.f planted, boxes of both
    kinds; faces with d == 0 planted: fluid cells at ambient itself, and pairs whose mean is ambient"""
    rng = np.random.default_rng(seed)
    shape = (Y, X)
    solid = (rng.random(shape) < 0.2).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.6, rng.choice(np.array([1, 2, 8, 255], np.uint8), shape), 0).astype(np.uint8)
    count[0, :] = count[-1, :] = 0
    count[:, 0] = count[:, -1] = 0
    T = (F32(ambient) + rng.standard_normal(shape).astype(F32) * F32(4)).astype(F32)
    hit = rng.random(shape) < 0.3
    T[hit] = F32(ambient)                       # d == 0 on the faces between two such cells and next to air
    T[2:Y - 2:5, 2:X - 2] = F32(ambient) + F32(1.5)      # pairs (y, y + 1) with mean ambient exactly
    T[3:Y - 2:5, 2:X - 2] = F32(ambient) - F32(1.5)
    T[count == 0] = F32(ambient)
    utmp, vtmp = (rng.standard_normal(shape).astype(F32) * 3 for _ in range(2))
    for a in (utmp, vtmp):
        hit = rng.random(shape) < 0.2
        a[hit] = rng.choice(np.array([-0.0, 0.0, 1e-30, -3.5], F32), int(hit.sum()))
    boxes = []
    for k in range(nboxes):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya, yb = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
        boxes.append((int(rng.integers(0, 2)), float(F32(rng.standard_normal() * 20)), (xa, ya, xb, yb)))
    if nboxes >= 5:
        boxes[1] = boxes[0]                                          # a duplicate
        boxes[2] = (href.RATE, 0.3, (1, 1, X - 2, Y - 2))            # the whole interior, over every other box
        boxes[3] = (href.FIX, -7.0, (X - 2, Y - 2, X - 2, Y - 2))    # the last cell
        boxes[4] = (href.FIX, ambient, boxes[0][2])                  # FIX behind RATE: back to ambient, d == 0 there
    return solid, count, T, utmp, vtmp, boxes


@pytest.mark.parametrize("size,nboxes,beta,kappa,acc", [((37, 23), 0, 0.5, 0.0, (0.0, -10.0)), ((37, 23), 7, -2.0, 0.3, (3.0, -8.0)), ((37, 23), 64, 0.5, 2.5, (-0.0, 0.0)),
                                                        ((37, 23), 64, 0.0, 2.5, (1e-3, 7.0)), ((131, 70), 0, 3.0, 0.3, (2.5, 0.0)), ((131, 70), 33, 0.5, 0.0, (0.0, -10.0)),
                                                        ((131, 70), 64, -2.0, 2.5, (-4.0, -9.81))])
def test_the_restatement_against_its_loop_twin(size, nboxes, beta, kappa, acc):
    X, Y = size
    for seed, ambient in ((0, 0.0), (1, 20.0)):
        solid, count, T, utmp, vtmp, boxes = random_scene(1000 * nboxes + seed, X, Y, nboxes, ambient)
        h = href.heat(ambient, beta, kappa)
        dt = float(F32(0.0371))
        a = [x.copy() for x in (T, utmp, vtmp)]
        b = [x.copy() for x in (T, utmp, vtmp)]
        href.after_transport_arrays(a[0], a[1], a[2], solid, count, h, boxes, dt, acc)
        href.after_transport_loop(b[0], b[1], b[2], solid, count, h, boxes, dt, acc)
        for x, y, n in zip(a, b, ("T", "utmp", "vtmp")):
            assert np.array_equal(bits(x), bits(y)), n
        lu, lv = fref.live_faces(solid, count)
        assert np.array_equal(bits(a[1])[~lu], bits(utmp)[~lu]) and np.array_equal(bits(a[2])[~lv], bits(vtmp)[~lv])      # a face that is not live is not touched
        assert (a[0][count == 0] == F32(ambient)).all()
        if beta == 0 or acc[0] == 0:      # u keeps its bits, planted -0.f included
            assert np.array_equal(bits(a[1]), bits(utmp)) and (bits(utmp)[lu] == 0x80000000).any()
        if beta == 0:
            assert np.array_equal(bits(a[2]), bits(vtmp))
        elif acc[1] != 0:
            changed = bits(a[2]) != bits(vtmp)
            assert changed.any() and (nboxes or (lv & ~changed).any())      # some live faces move; of the planted ones (no box has been over them) some keep their bits
            cn = count != 0
            both = np.zeros(cn.shape, bool)
            both[:-1] = cn[:-1] & cn[1:] & lv[:-1]
            zero = np.zeros(cn.shape, bool)
            zero[:-1] = (a[0][:-1] + a[0][1:]) / F32(2) == F32(ambient)
            assert not changed[both & zero].any()
            if kappa == 0 and not nboxes:
                assert (both & zero & (bits(vtmp) == 0x80000000)).any()      # a planted -0.f on a face with d == 0 stays -0.f


def test_fix_behind_rate_comes_out_in_list_order():
    count = np.zeros((8, 8), np.uint8)
    count[1:7, 1:7] = 1
    solid = np.zeros_like(count)
    z = np.zeros((8, 8), F32)
    for after in (href.after_transport_arrays, href.after_transport_loop):
        T = z.copy()
        after(T, z.copy(), z.copy(), solid, count, href.heat(), [(href.RATE, 10.0, (2, 2, 4, 4)), (href.FIX, 3.0, (3, 3, 5, 5)), (href.RATE, -1.0, (4, 4, 6, 6))], 0.1, (0, -10))
        assert T[2, 2] == F32(F32(10.0) * F32(0.1)) and T[3, 3] == 3 and T[4, 4] == F32(F32(3) + F32(F32(-1) * F32(0.1))) and T[6, 6] == F32(F32(-1) * F32(0.1)) and T[0, 0] == 0


# ----------------------------------------------------------------------------- layouts, sanitizers
def test_dtypes_are_the_structs(tmp_path):
    h, b = ea.HEAT_DTYPE, ea.HEAT_BOX_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d %d %d", sizeof(euler_heat), sizeof(euler_heat_box), (int)EULER_HEAT_BOXES_MAX, (int)EULER_HEAT_FIX, (int)EULER_HEAT_RATE);\n'
                   + "".join('  printf(" %%zu", offsetof(euler_heat, %s));\n' % n for n in h.names)
                   + "".join('  printf(" %%zu", offsetof(euler_heat_box, %s));\n' % n for n in b.names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:5] == [32, 24, 64, 0, 1] == [h.itemsize, b.itemsize, ea.HEAT_BOXES_MAX, ea.HEAT_FIX, ea.HEAT_RATE]
    assert out[5:12] == [h.fields[n][1] for n in h.names] == [0, 4, 8, 12, 16, 20, 24]
    assert out[12:] == [b.fields[n][1] for n in b.names] == [0, 4, 8, 12, 16, 20]
    assert [h.fields[n][0] for n in h.names] == [np.float32] * 4 + [np.int32] * 2 + [np.float64]
    assert [b.fields[n][0] for n in b.names] == [np.int32] * 4 + [np.float32, np.int32]
    d = ea.heat_default()
    assert d.dtype == h and not d.tobytes().strip(b"\0")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the check of the record and the list - every refusal, in order -, the box and value checks, the tile-table builder, the painter and the command's spec parsers"""
    exe = str(tmp_path / "sanitize_heat")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_heat.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- known answers on the CPU composition
SIZE = (64, 40)      # the half tank: water in rows 1 .. 19
HOT = (24, 6, 39, 13)      # a blob inside the water
HEATER = (href.FIX, 8.0, (26, 1, 37, 2))      # on the floor
STATE = ("u", "v", "count", "prev_count", "markers", "cr", "cg", "cb")


def blob(o, h, box, value):
    T = href.field(o, h)
    x0, y0, x1, y1 = box
    sub = T[y0:y1 + 1, x0:x1 + 1]
    sub[np.asarray(o.count)[y0:y1 + 1, x0:x1 + 1] != 0] = F32(value)
    return T


def state_bits(o):
    return [np.array(getattr(o, n)).view(np.uint8).copy() for n in STATE] + [int(o.c.rng_state), o.n_markers]


def same_state(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("h,hot", [(href.heat(1.0, 0.0, 0.4, 5.0), 9.0),      # beta == 0: a passive scalar, whatever it holds
                                   (href.heat(1.0, 3.0, 0.4, 1.0), 1.0)])     # beta = 3 over a field that is ambient everywhere (the source's water too)
def test_a_passive_or_uniform_field_leaves_the_run_untouched(am, h, hot):
    from euler_amd import scenarios
    for text, rk2, mc in ((scenarios.dam_break(), 0, 0), (scenarios.waterfall(), 1, 1)):
        a = Oracle(100, 40, rainbow=True).load_text(text, upscale=True)
        b = Oracle(100, 40, rainbow=True).load_text(text, upscale=True)
        T = blob(a, h, (1, 1, 98, 38), hot)
        if not h["beta"]:      # stripes, so that transport and diffusion have something to move
            ys, xs = np.indices(T.shape)
            T[np.asarray(a.count) != 0] += ((xs + ys) % 7).astype(F32)[np.asarray(a.count) != 0]
        boxes = [(href.FIX, hot, (5, 2, 20, 9)), (href.RATE, 0.0 if h["beta"] else 30.0, (10, 1, 50, 5))]
        for k in range(6):
            href.step(am, a, T, h, boxes, rk2=rk2, mc=mc)
            fref.step(am, b, fref.DEFAULT, [], fref.Clock(), rk2, mc)
            assert same_state(state_bits(a), state_bits(b)), (rk2, mc, k)
        if h["beta"]:
            assert (T == F32(1.0)).all()
        else:
            assert (T[np.asarray(a.count) == 0] == F32(1.0)).all() and (T != F32(1.0)).any()
            assert len(np.unique(T)) > 10 or mc      # (the waterfall's water all comes from the source: source_t)
        a.close(); b.close()


def test_diffusion_conserves_heat_in_a_still_tank(am):
    """The half tank without gravity is at rest bit for bit (test_forcing_host.py), so the transport returns every value as it is and only step c acts.  In exact
    arithmetic sum T is conserved: fl(T_n - T) = -fl(T - T_n), the exchanges cancel in pairs.  What does not cancel is the rounding of one cell's update: three
    rounded adds into acc (the first, to 0, is exact), each off by at most u |acc| <= u 8 M and scaled by c; the product fl(c acc), off by u c 8 M; the add
    T + ..., off by u M' with M' <= M - the step is a convex combination for c <= 0.25, so no value exceeds M = max |T| of the start by more than roundings
    (the factor 1.01).  Per cell and step at most u M (32 c + 1) 1.01, over N fluid cells and S steps N S times that.  The sums are taken in float64."""
    o = Oracle(*SIZE).load_half_tank()
    kappa = 2.5
    h = href.heat(0.0, 0.0, kappa)
    T = blob(o, h, HOT, 50.0)
    T[np.asarray(o.count) != 0] += F32(0.37)
    cn = np.asarray(o.count) != 0
    N, M, s0 = int(cn.sum()), float(np.abs(T).max()), float(T[cn].astype(np.float64).sum())
    f, clock = fref.forcing((0, 0)), fref.Clock()
    steps = 0
    for _ in range(8):
        n, _ = href.step(am, o, T, h, [], f, clock=clock)
        steps += n
    assert not bits(o.u).any() and not bits(o.v).any() and np.array_equal(np.asarray(o.count) != 0, cn)
    s1 = float(T[cn].astype(np.float64).sum())
    c = kappa * 0.1
    bound = N * steps * U24 * M * (32 * c + 1) * 1.01
    print("sum T %.9g -> %.9g over %d cells, %d substeps: off by %.3g, bound %.3g" % (s0, s1, N, steps, abs(s1 - s0), bound))
    assert steps == 8 and abs(s1 - s0) <= bound
    assert float(T.max()) < M and int((T[cn] > 0.371).sum()) > 16 * 8      # ... and it did diffuse
    o.close()


def test_maximum_principle(am):
    """beta == 0, RK1, no RATE box, kappa = 2.5: T stays between the smallest and the largest of the initial field, ambient, source_t and the FIX values, [lo, hi],
    widened per substep by what the float32 operations round, with A = max(|lo|, |hi|) and u = 2^-24:
      eu_interp: a lerp is fl(fl(fl(1 - f) x0) + fl(f x1)); the weights fl(1 - f) and f sum to 1 + d with |d| <= u, so the exact combination leaves [lo, hi] by
        at most u A, the two products and the add round by at most u A each: 4 u A per lerp, two levels of them: 8 u A.  A masked weight is 0 or 1 and a masked
        sample 0: 1 x + 0 0 is x, exact.  (With no valid corner at all the interpolation gives 0: ambient = 0 here, inside the range.)
      the extension: a sum of n <= 9 values and a division, at most 10 u A; the diffusion: a convex combination whose roundings are at most (32 c + 1) u A <= 9 u A
        (test_diffusion_conserves_heat_in_a_still_tank).
    32 u A per substep bounds them all; A may grow by these roundings: 1.001 A."""
    from euler_amd import scenarios
    o = Oracle(100, 40).load_text(scenarios.dam_break(), upscale=True)
    h = href.heat(0.0, 0.0, 2.5, -4.0)
    boxes = [(href.FIX, 6.0, (10, 1, 40, 6)), (href.FIX, -2.5, (30, 4, 60, 12))]      # on the floor the block falls on
    T = blob(o, h, (1, 1, 98, 38), -4.0)
    ys, xs = np.indices(T.shape)
    T[np.asarray(o.count) != 0] += ((xs + ys) % 11).astype(F32)[np.asarray(o.count) != 0]      # stripes over [-4, 6]
    assert T.min() == -4 and T.max() == 6
    lo, hi = -4.0, 6.0
    A, sub = 6.0 * 1.001, 0
    for k in range(20):
        n, _ = href.step(am, o, T, h, boxes)
        sub += n
        w = 32 * U24 * A * sub
        assert lo - w <= float(T.min()) and float(T.max()) <= hi + w, (k, T.min(), T.max(), w)
    cn = np.asarray(o.count) != 0
    assert np.abs(o.v).max() > 1 and np.abs(o.u).max() > 1 and len(np.unique(T[cn])) > 100 and sub > 20
    print("T in [%.9g, %.9g] after %d substeps, allowed widening %.3g" % (T.min(), T.max(), sub, w))
    o.close()


def closed_tank_text(X, Y):
    """solid walls all around, water everywhere inside"""
    wall, row = "X" * (X - 2), "X" + "0" * (X - 4) + "X"
    return "\n".join([wall] + [row] * (Y - 4) + [wall]) + "\n"


def centre_of_heat(o, T, ambient):
    cn = np.asarray(o.count) != 0
    d = np.abs(T.astype(np.float64) - ambient) * cn
    ys = np.arange(o.Y, dtype=np.float64)[:, None]
    return float((d * ys).sum() / d.sum())


@pytest.mark.parametrize("value,gy", [(5.0, -10.0), (-5.0, -10.0), (5.0, 10.0), (-5.0, 10.0)])
def test_a_hot_blob_rises_and_a_cold_one_sinks(am, value, gy):
    """signs only: in a closed tank full of water the centre of heat of a blob moves against gravity when it is hot, with gravity when it is cold"""
    X, Y = SIZE
    o = Oracle(X, Y).load_text(closed_tank_text(X, Y))
    assert int((np.asarray(o.count) != 0).sum()) == (X - 4) * (Y - 4) and int(np.asarray(o.solid).sum()) == 2 * (X - 2) + 2 * (Y - 4)
    h = href.heat(20.0, 0.5)
    T = blob(o, h, (24, 14, 39, 25), 20.0 + value)
    y0 = centre_of_heat(o, T, 20.0)
    f, clock = fref.forcing((0, gy)), fref.Clock()
    for _ in range(6):
        href.step(am, o, T, h, [], f, clock=clock)
    y1 = centre_of_heat(o, T, 20.0)
    print("blob %+g under gy %g: centre of heat y %.4f -> %.4f" % (value, gy, y0, y1))
    assert (y1 - y0) * value * -gy > 0 and abs(y1 - y0) > 0.05
    o.close()


def heater_flux(solid, count, u, v):
    _, _, (x0, y0, x1, y1) = HEATER
    rec = gref.gauge_ref(solid, count, u, v, None, gref.FLUX, (x0, y1 + 3, x1, y1 + 3))      # a row of v faces above the heater
    assert int(rec["fluid"]) == x1 - x0 + 1      # under water
    return gref.derive(rec, gref.FLUX)["b"]


def test_a_heater_on_the_floor_drives_an_upward_flux(am):
    o = Oracle(*SIZE).load_half_tank()
    h = href.heat(0.0, 0.5, 0.2)
    T = href.field(o, h)
    for _ in range(5):
        href.step(am, o, T, h, [HEATER])
    b = heater_flux(np.array(o.solid), np.array(o.count), np.array(o.u), np.array(o.v))
    print("flux through the row above the heater after 5 frames: %.6f" % b)
    assert b > 0
    o.close()


# ----------------------------------------------------------------------------- the raster's restatement and the painter (host only)
def random_heat_records(seed, h, w):
    rng = np.random.default_rng(seed)
    heat = np.zeros((h, w), href.PX_DTYPE)
    heat["cells"] = rng.integers(1, 50, (h, w))
    heat["water"] = np.minimum(rng.integers(0, 50, (h, w)), heat["cells"])
    heat["t_pos"] = rng.integers(0, 1 << 34, (h, w)) * (heat["water"] > 0)
    heat["t_neg"] = rng.integers(0, 1 << 34, (h, w)) * (heat["water"] > 0)
    heat["t_pos"][0, 0], heat["t_neg"][0, 0] = 4096 << 20, 0      # the clamp of an infinity, in one water cell
    heat["water"][0, 0] = 1
    return heat


def test_the_rasters_restatement_on_planted_values():
    """NaN to no sum and no maximum (the cell still counts as water), an infinity as the clamp's 4096 in the sums and itself in the maxima, -0.f on the positive side"""
    count = np.ones((6, 8), np.uint8)
    solid, sink = np.zeros_like(count), np.zeros_like(count)
    solid[2, 2], sink[3, 3], count[4, 4] = 1, 1, 0
    T = np.full((6, 8), 2.0, F32)
    T[1, 1], T[1, 2], T[1, 3], T[1, 4], T[1, 5], T[1, 6] = np.nan, np.inf, -np.inf, 5000.0, 1.5, 3.25
    r = href.raster(T, solid, sink, count, 2.0, (1, 1, 6, 4), 1, 1)[0, 0]
    assert (int(r["cells"]), int(r["water"])) == (24, 21)
    assert int(r["t_pos"]) == (4096 << 20) + (4096 << 20) + int(1.25 * (1 << 20)) and int(r["t_neg"]) == (4096 << 20) + (1 << 19)
    assert r["max_above"] == np.inf and r["max_below"] == np.inf
    r = href.raster(T, solid, sink, count, 2.0, (4, 1, 6, 1), 3, 1)[0]
    assert [int(t) for t in r["t_pos"]] == [4096 << 20, 0, int(1.25 * (1 << 20))] and r["max_above"].tolist() == [4998.0, 0.0, 1.25] and r["max_below"].tolist() == [0.0, 0.5, 0.0]


@pytest.mark.parametrize("scale", [0.5, 3.0, 4096.0])
def test_the_painter_against_numpy(scale):
    heat = random_heat_records(3, 5, 7)
    px = np.zeros((5, 7), ea.OVERVIEW_DTYPE)
    px["cells"], px["water"] = heat["cells"], heat["water"]
    px["dye"] = 7
    got = ea.heat_paint(heat, px, 20.0, scale)
    assert np.array_equal(got["dye"], href.paint(heat, scale))
    for n in px.dtype.names:
        if n != "dye":
            assert np.array_equal(got[n], px[n])
    assert len(np.unique(got["dye"])) > 10 and (got["dye"][heat["water"] == 0] == 0).all()
    # its refusals are euler_flow_paint's: a null pointer, W or H < 1, a scale that is not finite and positive, records of another raster; px unchanged
    L = ea.load_library()
    call = lambda h, p, w, hh, amb, sc: L.euler_heat_paint(h, p, w, hh, amb, sc)
    work = px.copy()
    hp, pp = heat.ctypes.data, work.ctypes.data
    assert call(None, pp, 7, 5, 0.0, 1.0) == -1 and call(hp, None, 7, 5, 0.0, 1.0) == -1 and call(hp, pp, 0, 5, 0.0, 1.0) == -1 and call(hp, pp, 7, 0, 0.0, 1.0) == -1
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(hp, pp, 7, 5, 0.0, float(bad)) == -1
    assert call(hp, pp, 7, 5, float(np.nan), 1.0) == -1
    other = heat.copy()
    other["water"][4, 6] += 1
    assert call(other.ctypes.data, pp, 7, 5, 0.0, 1.0) == -1
    other = heat.copy()
    other["cells"][2, 3] += 1
    assert call(other.ctypes.data, pp, 7, 5, 0.0, 1.0) == -1
    assert work.tobytes() == px.tobytes()
    assert ea.HEAT_PX_DTYPE == href.PX_DTYPE
