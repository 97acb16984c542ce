"""The host half of the observer passes on row slabs (docs/observer_passes.md "On row slabs"), no GPU: the planners of csrc/euler_host.c - the clipped row range of
a rank, the pixel rows of every rank, the all-gather offsets and counts, the contributors of a pixel row, the per-rank gauge chunk tables - against brute-force Python
loops on random partitions, boxes and rasters, and the same code under the sanitizers in a stand-alone program (tests/c/sanitize_slab_observers.c)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import euler_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXR = 16
EULER_EINVAL = -1


class Plan(C.Structure):      # eu_slab_plan (csrc/euler_host.h)
    _fields_ = [("nranks", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("y0", C.c_int32), ("y1", C.c_int32),
                ("ya", C.c_int32 * MAXR), ("yb", C.c_int32 * MAXR), ("p_lo", C.c_int32 * MAXR), ("p_hi", C.c_int32 * MAXR),
                ("off", C.c_int64 * MAXR), ("cnt", C.c_int64 * MAXR), ("total", C.c_int64)]


class Chunk(C.Structure):     # eu_gauge_chunk
    _fields_ = [(n, C.c_int32) for n in ("gauge", "kind", "x0", "y0", "x1", "y1")]


@pytest.fixture(scope="module")
def L():
    lib = ea.load_library()
    i32, p32, p64 = C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    lib.eu_slab_clip_rows.argtypes, lib.eu_slab_clip_rows.restype = [i32, i32, i32, i32, i32, p32, p32], C.c_int
    lib.eu_slab_plan_raster.argtypes, lib.eu_slab_plan_raster.restype = [C.POINTER(Plan), i32, p32, p32, i32, i32, i32, i32, i32], C.c_int
    lib.eu_slab_plan_flat.argtypes, lib.eu_slab_plan_flat.restype = [C.POINTER(Plan), i32, i32], C.c_int
    lib.eu_slab_plan_bytes.argtypes, lib.eu_slab_plan_bytes.restype = [C.POINTER(Plan), C.c_int64, p64, p64], None
    lib.eu_slab_plan_contributors.argtypes, lib.eu_slab_plan_contributors.restype = [C.POINTER(Plan), i32, p32, p32], C.c_int
    lib.eu_gauge_chunks_bands.argtypes, lib.eu_gauge_chunks_bands.restype = [C.c_void_p, i32, i32, i32, C.c_void_p], C.c_size_t
    lib.eu_gauge_chunks.argtypes, lib.eu_gauge_chunks.restype = [C.c_void_p, i32, C.c_void_p], C.c_size_t
    return lib


def random_partition(rng, nb, R, even):
    if even:
        return [(nb * r // R, nb * (r + 1) // R) for r in range(R)]      # euler_amd.slab.slab_bands
    cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, nb), R - 1, replace=False)) + [nb]
    return list(zip(cuts[:-1], cuts[1:]))


def random_case(rng):
    R = int(rng.integers(1, 9))
    nb = int(rng.integers(R, R + 12))
    Y = 64 * (nb - 1) + int(rng.integers(1, 64))      # a last band of 1 ... 63 rows
    if Y < 3:
        Y, nb = 3, 1
    part = random_partition(rng, nb, R, bool(rng.integers(0, 2)))
    y0, y1 = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
    Bh = y1 - y0 + 1
    t = rng.random()      # H = Bh, a few pixel rows (several ranks share one), anything
    H = Bh if t < 0.2 else (int(rng.integers(1, min(Bh, 4) + 1)) if t < 0.5 else int(rng.integers(1, Bh + 1)))
    return R, Y, part, y0, y1, int(rng.integers(1, 50)), H


def plan_of(L, R, Y, part, y0, y1, W, H):
    lo = (C.c_int32 * R)(*[p[0] for p in part])
    hi = (C.c_int32 * R)(*[p[1] for p in part])
    P = Plan()
    assert L.eu_slab_plan_raster(C.byref(P), R, lo, hi, Y, y0, y1, W, H) == 0
    return P


def test_the_raster_plan_against_brute_force_loops(L):
    rng = np.random.default_rng(20240)
    shared = thin = 0
    for _ in range(200):
        R, Y, part, y0, y1, W, H = random_case(rng)
        P = plan_of(L, R, Y, part, y0, y1, W, H)
        Bh = y1 - y0 + 1
        # the brute force: every row of the grid to its owner, every row of the box to its pixel row (the kernels' own formula)
        owner = np.full(Y, -1)
        for r, (lo, hi) in enumerate(part):
            owner[64 * lo:min(64 * hi, Y)] = r
        assert (owner >= 0).all()
        rows_of = [[y for y in range(y0, y1 + 1) if owner[y] == r] for r in range(R)]
        py_of = {y: ((y1 - y + 1) * H - 1) // Bh for y in range(y0, y1 + 1)}
        # 1. the union of the ranks' clipped rows is the box's rows, each once
        seen = []
        for r in range(R):
            ya, yb = C.c_int32(), C.c_int32()
            some = L.eu_slab_clip_rows(part[r][0], part[r][1], Y, y0, y1, C.byref(ya), C.byref(yb))
            assert (ya.value, yb.value) == (P.ya[r], P.yb[r]) and bool(some) == bool(rows_of[r])
            assert list(range(P.ya[r], P.yb[r] + 1)) == rows_of[r]
            seen += rows_of[r]
        assert seen == list(range(y0, y1 + 1))
        # 2. every rank's pixel rows are the ones its rows touch; every pixel row's contributors are the ranks whose rows intersect it
        for r in range(R):
            touched = sorted({py_of[y] for y in rows_of[r]})
            assert touched == list(range(P.p_lo[r], P.p_hi[r] + 1)), (r, touched, P.p_lo[r], P.p_hi[r])
        for py in range(H):
            want = sorted({int(owner[y]) for y in range(y0, y1 + 1) if py_of[y] == py})
            f, l = C.c_int32(), C.c_int32()
            assert L.eu_slab_plan_contributors(C.byref(P), py, C.byref(f), C.byref(l)) == 0
            assert list(range(f.value, l.value + 1)) == want, (py, want, f.value, l.value)
            shared += len(want) > 2
        thin += any(len(rows) == 1 for rows in rows_of)
        # 3. the offsets tile the staging area without gaps, rank after rank; the byte form is the record form times the record's size
        at = 0
        for r in range(R):
            assert P.off[r] == at and P.cnt[r] == len(set(py_of[y] for y in rows_of[r])) * W
            at += P.cnt[r]
        assert P.total == at <= (H + R - 1) * W
        off, cnt = (C.c_int64 * MAXR)(), (C.c_int64 * MAXR)()
        L.eu_slab_plan_bytes(C.byref(P), 48, off, cnt)
        assert [off[r] for r in range(R)] == [48 * P.off[r] for r in range(R)] and [cnt[r] for r in range(R)] == [48 * P.cnt[r] for r in range(R)]
    assert shared > 0 and thin > 0      # the cases reached a pixel row that more than two ranks share and a rank with one row of the box


def test_the_flat_plan_and_the_refusals(L):
    P = Plan()
    for R in range(1, 9):
        assert L.eu_slab_plan_flat(C.byref(P), R, 1024) == 0
        assert [P.off[r] for r in range(R)] == [1024 * r for r in range(R)] and [P.cnt[r] for r in range(R)] == [1024] * R and P.total == 1024 * R
        f, l = C.c_int32(), C.c_int32()
        assert L.eu_slab_plan_contributors(C.byref(P), 0, C.byref(f), C.byref(l)) == 0 and (f.value, l.value) == (0, R - 1)
    assert L.eu_slab_plan_flat(C.byref(P), 0, 1) == EULER_EINVAL and L.eu_slab_plan_flat(C.byref(P), 17, 1) == EULER_EINVAL and L.eu_slab_plan_flat(C.byref(P), 2, 0) == EULER_EINVAL
    lo, hi = (C.c_int32 * 2)(0, 2), (C.c_int32 * 2)(2, 4)
    ok = (2, lo, hi, 256, 1, 254, 4, 4)
    assert L.eu_slab_plan_raster(C.byref(P), *ok) == 0
    for k, bad in ((0, 0), (0, 17), (3, 0), (4, -1), (5, 256), (6, 0), (7, 0), (7, 255)):      # ranks, grid, box, raster
        args = list(ok)
        args[k] = bad
        assert L.eu_slab_plan_raster(C.byref(P), *args) == EULER_EINVAL, (k, bad)
    assert L.eu_slab_plan_raster(C.byref(P), 2, (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(2, 4), 256, 1, 254, 4, 4) == EULER_EINVAL      # overlapping band ranges


def test_the_ranks_chunk_tables_are_a_partition_of_the_whole_grid_table(L):
    rng = np.random.default_rng(7)
    for _ in range(60):
        R, Y, part, _, _, _, _ = random_case(rng)
        X = int(rng.integers(3, 400))
        n = int(rng.integers(1, 12))
        g = np.zeros(n, ea.GAUGE_DTYPE)
        for k in range(n):
            xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
            ya, yb = sorted(int(t) for t in rng.integers(1, Y - 1, 2))
            g[k] = (int(rng.integers(0, 4)), xa, ya, xb, yb, 0)
        m = L.eu_gauge_chunks(g.ctypes.data, n, None)
        whole = (Chunk * max(m, 1))()
        assert L.eu_gauge_chunks(g.ctypes.data, n, C.addressof(whole)) == m
        as_tuple = lambda c: (c.gauge, c.kind, c.x0, c.y0, c.x1, c.y1)
        want = [as_tuple(whole[k]) for k in range(m)]
        assert len(set(want)) == m
        got = []
        for lo, hi in part:
            mr = L.eu_gauge_chunks_bands(g.ctypes.data, n, lo, hi, None)
            mine = (Chunk * max(mr, 1))()
            assert L.eu_gauge_chunks_bands(g.ctypes.data, n, lo, hi, C.addressof(mine)) == mr
            t = [as_tuple(mine[k]) for k in range(mr)]
            assert all(lo <= c[3] >> 6 and c[5] >> 6 < hi for c in t)      # every chunk in the rank's own bands
            assert t == [c for c in want if lo <= c[3] >> 6 < hi]          # ... and in the whole table's order
            got += t
        assert sorted(got) == sorted(want)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the planners: random and degenerate input"""
    exe = str(tmp_path / "sanitize_slab_observers")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "sanitize_slab_observers.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
