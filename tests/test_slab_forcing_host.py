"""The host half of forcing and temperature on row slabs (docs/forcing.md, docs/heat.md "On row slabs"), no GPU: the band-filtered tile table of a box list
(eu_force_tiles_bands, csrc/euler_host.c) against brute force - every band range, the union over a partition, each entry on exactly one rank -, the digests the
ranks compare before euler_set_forcing / euler_set_heat change anything, and the same code under the sanitizers in a stand-alone program
(tests/c/sanitize_slab_forcing.c)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import euler_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = np.dtype([("tx", np.int32), ("ty", np.int32), ("boxes", np.uint64)])      # eu_force_tile (csrc/euler_host.h)
SIZES = [(103, 150), (200, 192), (264, 136)]


@pytest.fixture(scope="module")
def L():
    lib = ea.load_library()
    i32, vp = C.c_int32, C.c_void_p
    lib.eu_force_tiles.argtypes, lib.eu_force_tiles.restype = [vp, C.c_size_t, i32, i32, i32, vp], C.c_size_t
    lib.eu_force_tiles_bands.argtypes, lib.eu_force_tiles_bands.restype = [vp, C.c_size_t, i32, i32, i32, i32, i32, vp], C.c_size_t
    lib.eu_forcing_digest.argtypes, lib.eu_forcing_digest.restype = [vp, vp], C.c_uint64
    lib.eu_heat_digest.argtypes, lib.eu_heat_digest.restype = [vp, vp], C.c_uint64
    return lib


def table(L, boxes, X, Y, lo=None, hi=None):
    """the tile table of a list, whole (lo is None) or of the bands [lo, hi): counted first, then written into a buffer of exactly that many entries"""
    p = boxes.ctypes.data if len(boxes) else None
    args = (p, boxes.dtype.itemsize, len(boxes), X, Y) + (() if lo is None else (lo, hi))
    fn = L.eu_force_tiles if lo is None else L.eu_force_tiles_bands
    n = fn(*args, None)
    out = np.zeros(n + 1, TILE)
    out[n] = (-7, -7, 0xdeadbeef)      # a sentinel behind the last entry
    assert fn(*args, out.ctypes.data) == n and tuple(out[n]) == (-7, -7, 0xdeadbeef)
    return out[:n]


def brute(boxes, X, Y, lo, hi):
    """tile rows lo ... hi - 1, row by row, a tile with the bit set of the boxes that touch it"""
    out = []
    for ty in range(lo, min(hi, (Y + 63) // 64)):
        for tx in range((X + 63) // 64):
            s = 0
            for k, b in enumerate(boxes):
                if b["x0"] <= 64 * tx + 63 and b["x1"] >= 64 * tx and b["y0"] <= 64 * ty + 63 and b["y1"] >= 64 * ty:
                    s |= 1 << k
            if s:
                out.append((tx, ty, s))
    return out


def random_boxes(rng, X, Y, n):
    b = np.zeros(n, ea.FORCE_BOX_DTYPE)
    for k in range(n):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya, yb = sorted(int(t) for t in rng.integers(1, min(Y - 1, 1 + int(rng.integers(2, Y))), 2))      # (half the lists keep to the lower rows: bands no box touches)
        b[k] = (xa, ya, xb, yb, float(rng.standard_normal()), float(rng.standard_normal()))
    planted = [(5, 63, 9, 64), (X - 2, 127, X - 2, 128) if Y > 130 else (X - 2, 60, X - 2, 70), (3, Y - 2, 7, Y - 2), (1, Y - 3, X - 2, Y - 2)]
    for k, box in enumerate(planted):      # across rows 63|64 and 127|128, touching Y - 2 in the last band
        if 2 * k + 1 < n:
            b[2 * k + 1] = box + (1.0, -1.0)
    return b


@pytest.mark.parametrize("X,Y", SIZES)
def test_band_filter_against_brute_force(L, X, Y):
    rng = np.random.default_rng(X * 1000 + Y)
    nb = (Y + 63) // 64
    empty_seen = False
    for n in list(range(0, 65, 7)) + [64, 1, 2]:
        boxes = random_boxes(rng, X, Y, n)
        whole = table(L, boxes, X, Y)
        assert [tuple(int(v) for v in e) for e in whole] == brute(boxes, X, Y, 0, nb)
        for lo in range(nb + 1):
            for hi in range(lo, nb + 1):
                got = [tuple(int(v) for v in e) for e in table(L, boxes, X, Y, lo, hi)]
                assert got == brute(boxes, X, Y, lo, hi), (n, lo, hi)
                empty_seen = empty_seen or (n > 0 and hi > lo and not got)
        # every partition into consecutive band ranges: the ranks' tables, rank after rank, ARE the whole table - each entry on exactly one rank
        for cuts in ([0, nb], [0, 1, nb], list(range(nb + 1))):
            parts = [table(L, boxes, X, Y, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.array_equal(np.concatenate(parts), whole), (n, cuts)
    assert empty_seen      # a range no box touches gave 0 entries
    # one box on a single rank: the others get nothing
    one = np.zeros(1, ea.FORCE_BOX_DTYPE)
    one[0] = (2, 70, 9, 80, 1.0, 0.0)
    assert len(table(L, one, X, Y, 0, 1)) == 0 and len(table(L, one, X, Y, 1, 2)) == 1 and len(table(L, one, X, Y, 2, nb)) == 0
    last = np.zeros(1, ea.FORCE_BOX_DTYPE)
    last[0] = (X - 2, Y - 2, X - 2, Y - 2, 1.0, 0.0)      # the last cell lies in the last band, however few rows it has
    assert len(table(L, last, X, Y, 0, nb - 1)) == 0 and [tuple(int(v) for v in e) for e in table(L, last, X, Y, nb - 1, nb)] == [((X - 2) // 64, nb - 1, 1)]


def test_the_filter_serves_heat_boxes_by_their_stride(L):
    X, Y = 200, 192
    rng = np.random.default_rng(5)
    fb = random_boxes(rng, X, Y, 20)
    hb = np.zeros(20, ea.HEAT_BOX_DTYPE)
    for n in ("x0", "y0", "x1", "y1"):
        hb[n] = fb[n]
    hb["value"], hb["kind"] = 3.0, ea.HEAT_RATE
    for lo, hi in ((0, 1), (1, 3), (0, 3), (2, 2)):
        assert np.array_equal(table(L, hb, X, Y, lo, hi), table(L, fb, X, Y, lo, hi))


def forcing_pair(rng, n):
    f = ea.forcing_record((1.5, -9.0), (0.5, 0.25, 2.0, 0.125), n)
    b = np.zeros(ea.FORCE_BOXES_MAX, ea.FORCE_BOX_DTYPE)      # every slot filled: the ones beyond n must not count
    for k in range(len(b)):
        b[k] = (1 + k, 2 + k, 70 + k, 80 + k, float(rng.standard_normal()), float(rng.standard_normal()))
    return f, b


def test_forcing_digest(L):
    rng = np.random.default_rng(11)
    dig = lambda f, b: L.eu_forcing_digest(f.ctypes.data, b.ctypes.data)
    seen = set()
    for n in (0, 1, 5, 64):
        f, b = forcing_pair(rng, n)
        d = dig(f, b)
        assert d == dig(f.copy(), b.copy())      # equal for equal lists
        seen.add(d)
        for name in ("gx", "gy", "shake_x", "shake_y", "shake_hz", "shake_phase"):      # any field of the record
            g = f.copy()
            g[name] += 1
            assert dig(g, b) != d, name
        for k in range(n):      # any field of any box
            for name in ea.FORCE_BOX_DTYPE.names:
                c = b.copy()
                c[name][k] += 1
                assert dig(f, c) != d, (k, name)
        if n >= 2:      # two boxes swap places
            c = b.copy()
            c[[0, n - 1]] = c[[n - 1, 0]]
            assert dig(f, c) != d
        if n < 64:      # slots beyond nboxes do not change it
            c = b.copy()
            c[n:] = 0
            assert dig(f, c) == d
            g = f.copy()
            g["nboxes"] = n + 1      # ... but one box more does
            assert dig(g, b) != d
    assert len(seen) == 4
    f, b = forcing_pair(rng, 0)
    assert L.eu_forcing_digest(f.ctypes.data, None) == dig(f, b)
    z, m = f.copy(), f.copy()
    z["gx"], m["gx"] = 0.0, -0.0
    assert dig(z, b) != dig(m, b)      # (the bytes are compared: -0.f is not +0.f)


def test_heat_digest(L):
    dig = lambda h, b: L.eu_heat_digest(h.ctypes.data if h is not None else None, b.ctypes.data if b is not None else None)
    h = ea.heat_default()
    h["ambient"], h["beta"], h["kappa"], h["source_t"], h["nboxes"] = 1.0, 0.5, 0.25, 3.0, 3
    b = np.zeros(ea.HEAT_BOXES_MAX, ea.HEAT_BOX_DTYPE)
    for k in range(len(b)):
        b[k] = (1 + k, 1 + k, 9 + k, 9 + k, float(k), ea.HEAT_FIX if k % 2 else ea.HEAT_RATE)
    d = dig(h, b)
    assert d == dig(h.copy(), b.copy())
    for name in ("ambient", "beta", "kappa", "source_t"):
        g = h.copy()
        g[name] += 1
        assert dig(g, b) != d, name
    for k in range(3):
        for name in ea.HEAT_BOX_DTYPE.names:
            c = b.copy()
            c[name][k] += 1
            assert dig(h, c) != d, (k, name)
    c = b.copy()
    c[[0, 2]] = c[[2, 0]]
    assert dig(h, c) != d
    c = b.copy()
    c[3:] = 0
    assert dig(h, c) == d
    off = dig(None, None)      # switching off has a digest of its own, whatever list comes with it
    assert off == dig(None, b) and off != d
    g = ea.heat_default()
    assert off != dig(g, None)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the band-filtered tile table and the two digests"""
    exe = str(tmp_path / "sanitize_slab_forcing")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "sanitize_slab_forcing.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
